// Training-side kernels: GRC weight-fold backward, fused GAN / L1 / hinge losses (value + gradient in one pass),
// log-mel spectrogram loss (forward + backward), flat-arena AdamW, the weight EMA on the arena and the multi-tensor gradient gather.
//   losses:   hifigan_modified/complete_vocoder.py:89-184 (LSGAN + L1), conditioned_hifigan.py:254-267 (hinge)
//   AdamW:    conditioned_hifigan.py:219 (torch.optim.AdamW semantics: decoupled weight decay, bias correction)
//   mel loss: defined by this build (the reference only has placeholders)
#include "common.h"
#include "philox.h"
#include <cstdlib>

namespace mv {

// ------------------------------------------------------------------------------------------- dropout keep-mask (Philox4x32-10)
// mask[i] = 1 with probability 1-p (nn.Dropout of grc_lora.py:151,162).  Counter-based: element block i/8 is counter (i/8, 0, 0, 0)
// under key (seed lo, seed hi), 16 random bits per element - the mask depends only on (seed, index), not on the launch geometry.
// philox4x32_10 itself is in philox.h (the clip sampler's noise draws from it too).
__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ mask, long n, uint32_t thresh16, uint32_t k0, uint32_t k1) {
  const long nblk = (n + 7) / 8;
  for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblk; blk += (long)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), 0u, 0u, k0, k1, r);
    uint8_t m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = ((r[e >> 1] >> (16 * (e & 1))) & 0xffffu) >= thresh16 ? 1 : 0;   // keep iff u >= p
    if (blk * 8 + 8 <= n) *reinterpret_cast<uint2*>(mask + blk * 8) = *reinterpret_cast<const uint2*>(m);
    else for (int e = 0; blk * 8 + e < n; ++e) mask[blk * 8 + e] = m[e];
  }
}

// Counter-offset form of the same mask: counter (blk lo, blk hi, ctr lo, ctr hi) - ctr = 0 gives dropout_mask_kernel's bits.  With
// `state` set, {key, ctr_base} (int64) come from device memory and ctr = ctr_base + `ctr` (the mask's slot in the step): a captured
// HIP graph then draws new masks whenever the host advances ctr_base between replays.
__global__ __launch_bounds__(256) void dropout_mask_ctr_kernel(uint8_t* __restrict__ mask, long n, uint32_t thresh16,
                                                               const long long* __restrict__ state, uint64_t key, uint64_t ctr) {
  if (state) { key = (uint64_t)state[0]; ctr += (uint64_t)state[1]; }
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32), c2 = (uint32_t)ctr, c3 = (uint32_t)(ctr >> 32);
  const long nblk = (n + 7) / 8;
  for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblk; blk += (long)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), c2, c3, k0, k1, r);
    uint8_t m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = ((r[e >> 1] >> (16 * (e & 1))) & 0xffffu) >= thresh16 ? 1 : 0;   // keep iff u >= p
    if (blk * 8 + 8 <= n) *reinterpret_cast<uint2*>(mask + blk * 8) = *reinterpret_cast<const uint2*>(m);
    else for (int e = 0; blk * 8 + e < n; ++e) mask[blk * 8 + e] = m[e];
  }
}

// ------------------------------------------------------------------------------------------- GRC fold backward
// forward (norm_elem.hip grc_fold_kernel): comb[o'][c][j] = [c in grp(o')] Wc[o'][c_loc][j] + [j==mid] s (A B)[c][o']
//   w_eff[o][c][j] = sum_o' Wp[o][o'] comb[o'][c][j];  b_eff[o] = sum_o' Wp[o][o'] bc[o'] + bp[o]
template <typename P>
__global__ __launch_bounds__(1024) void grc_fold_bwd_kernel(const float* __restrict__ g_weff, const float* __restrict__ g_beff,
                                                           const P* __restrict__ conv_w, const P* __restrict__ conv_b,
                                                           const P* __restrict__ A, const P* __restrict__ Bm,
                                                           const P* __restrict__ scal, const P* __restrict__ proj_w,
                                                           float* __restrict__ g_conv_w, float* __restrict__ g_conv_b,
                                                           float* __restrict__ g_A, float* __restrict__ g_B,
                                                           float* __restrict__ g_s, float* __restrict__ g_proj_w,
                                                           float* __restrict__ g_proj_b, int Cin, int Cout, int ks,
                                                           int groups, int rank) {
  extern __shared__ float sm[];
  float* gcomb = sm;                         // [Cout][Cin][ks]
  float* L = gcomb + Cout * Cin * ks;        // [Cin][Cout]
  float* red = L + Cin * Cout;               // [32]
  float* gwl = red + 32;                     // [Cout][Cin][ks] copy of g_weff: every later loop re-reads it many times
  const int tid = threadIdx.x, nt = blockDim.x;
  const int cin_g = Cin / groups, cout_g = Cout / groups, mid = ks / 2;
  // parameter copies in LDS: the loops below are chains of dependent reads (192 per g_proj_w element) - out of global memory
  // each link was an L2 round trip (44 us for the whole kernel)
  float* Wl = gwl + Cout * Cin * ks;         // conv_w [Cout][cin_g][ks]
  float* Pl = Wl + Cout * cin_g * ks;        // proj_w [Cout][Cout]
  float* Al = Pl + Cout * Cout;              // A [Cin][rank]
  float* Bl = Al + Cin * rank;               // B [rank][Cout]
  const float s = ld<P>(scal);
  for (int i = tid; i < Cout * Cin * ks; i += nt) gwl[i] = g_weff[i];
  for (int i = tid; i < Cout * cin_g * ks; i += nt) Wl[i] = ld<P>(conv_w + i);
  for (int i = tid; i < Cout * Cout; i += nt) Pl[i] = ld<P>(proj_w + i);
  for (int i = tid; i < Cin * rank; i += nt) Al[i] = ld<P>(A + i);
  for (int i = tid; i < rank * Cout; i += nt) Bl[i] = ld<P>(Bm + i);
  __syncthreads();
  for (int i = tid; i < Cin * Cout; i += nt) {
    const int c = i / Cout, o = i % Cout;
    float l = 0.f;
    for (int r = 0; r < rank; ++r) l += Al[c * rank + r] * Bl[r * Cout + o];
    L[i] = l;
  }
  for (int i = tid; i < Cout * Cin * ks; i += nt) {
    const int j = i % ks, c = (i / ks) % Cin, op = i / (ks * Cin);
    float a = 0.f;
    for (int o = 0; o < Cout; ++o) a += Pl[o * Cout + op] * gwl[(o * Cin + c) * ks + j];
    gcomb[i] = a;
  }
  __syncthreads();
  // proj_w / proj_b / conv_b
  for (int i = tid; i < Cout * Cout; i += nt) {
    const int o = i / Cout, op = i % Cout;
    const int g = op / cout_g;
    float a = g_beff[o] * ld<P>(conv_b + op);
    for (int c = 0; c < Cin; ++c)
      for (int j = 0; j < ks; ++j) {
        float comb = 0.f;
        if (c / cin_g == g) comb = Wl[(op * cin_g + (c - g * cin_g)) * ks + j];
        if (j == mid) comb += s * L[c * Cout + op];
        a += gwl[(o * Cin + c) * ks + j] * comb;
      }
    g_proj_w[i] = a;
  }
  for (int o = tid; o < Cout; o += nt) {
    g_proj_b[o] = g_beff[o];
    float a = 0.f;
    for (int oo = 0; oo < Cout; ++oo) a += Pl[oo * Cout + o] * g_beff[oo];
    g_conv_b[o] = a;
  }
  for (int i = tid; i < Cout * cin_g * ks; i += nt) {
    const int j = i % ks, cl = (i / ks) % cin_g, op = i / (ks * cin_g);
    const int c = (op / cout_g) * cin_g + cl;
    g_conv_w[i] = gcomb[((long)op * Cin + c) * ks + j];
  }
  for (int i = tid; i < Cin * rank; i += nt) {
    const int c = i / rank, r = i % rank;
    float a = 0.f;
    for (int op = 0; op < Cout; ++op) a += s * gcomb[((long)op * Cin + c) * ks + mid] * Bl[r * Cout + op];
    g_A[i] = a;
  }
  for (int i = tid; i < rank * Cout; i += nt) {
    const int r = i / Cout, op = i % Cout;
    float a = 0.f;
    for (int c = 0; c < Cin; ++c) a += Al[c * rank + r] * s * gcomb[((long)op * Cin + c) * ks + mid];
    g_B[i] = a;
  }
  float part = 0.f;
  for (int i = tid; i < Cin * Cout; i += nt) {
    const int c = i / Cout, op = i % Cout;
    part += L[i] * gcomb[((long)op * Cin + c) * ks + mid];
  }
  part = block_sum(part, red);
  if (tid == 0) g_s[0] = part;
}

// ------------------------------------------------------------------------------------------- losses (value + gradient)
// kind 0: mean((x-c)^2)            (LSGAN, complete_vocoder.py:104,157-158)
// kind 1: mean(|x-y|)              (L1 / "feature matching", :118,127)          gy (optional) = -gx
// kind 2: mean(relu(1 - x))        (hinge generator, conditioned_hifigan.py:263)
// kind 3: mean(relu(1 + x))        (hinge discriminator-fake, :265)
// kind 4: mean((x-y)^2)            (MSE between tensors, conditioned_hifigan.py:238)
// loss_acc[0] += weight * value ; gx = weight * d value / dx
template <typename T>
__global__ __launch_bounds__(256) void loss_kernel(const T* __restrict__ x, const T* __restrict__ y, float c, float weight,
                                                   float* __restrict__ loss_acc, T* __restrict__ gx, T* __restrict__ gy,
                                                   long n, int kind) {
  __shared__ float red[32];
  const float inv = weight / (float)n;
  float s = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = ld<T>(x + i);
    float l, g;
    if (kind == 0) { const float d = v - c; l = d * d; g = 2.f * d; }
    else if (kind == 1) { const float d = v - ld<T>(y + i); l = fabsf(d); g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    else if (kind == 2) { const float d = 1.f - v; l = d > 0.f ? d : 0.f; g = d > 0.f ? -1.f : 0.f; }
    else if (kind == 3) { const float d = 1.f + v; l = d > 0.f ? d : 0.f; g = d > 0.f ? 1.f : 0.f; }
    else { const float d = v - ld<T>(y + i); l = d * d; g = 2.f * d; }
    s += l;
    if (gx) st<T>(gx + i, g * inv);
    if (gy) st<T>(gy + i, -g * inv);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) atomicAdd(loss_acc, s * inv);
}

template <typename T>
__global__ __launch_bounds__(256) void scale_kernel(T* __restrict__ x, const float* __restrict__ factor_dev, float factor, long n) {
  const float f = factor_dev ? factor * factor_dev[0] : factor;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    st<T>(x + i, ld<T>(x + i) * f);
}

template <typename T>
__global__ __launch_bounds__(256) void scale_to_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ factor_dev,
                                                       float factor, long n) {
  const float f = factor_dev ? factor * factor_dev[0] : factor;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    st<T>(y + i, ld<T>(x + i) * f);
}

// ------------------------------------------------------------------------------------------- feature matching over hidden maps
// Defined by this build: complete_vocoder.py:118,127 take the L1 of the discriminators' outputs only; these two
// kernels extend that term to every hidden feature map, which lives in the stack's channels-last buffers (disc_fused.py).
// 16 bytes of T <-> floats (p 16-byte aligned)
template <typename T> __device__ __forceinline__ void ld16(const T* p, float* o) {
  constexpr int V = 16 / (int)sizeof(T);
  alignas(16) T tmp[V];
  *reinterpret_cast<uint4*>(tmp) = *reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int e = 0; e < V; ++e) o[e] = ld<T>(tmp + e);
}
template <typename T> __device__ __forceinline__ void st16(T* p, const float* v) {
  constexpr int V = 16 / (int)sizeof(T);
  alignas(16) T tmp[V];
#pragma unroll
  for (int e = 0; e < V; ++e) st<T>(tmp + e, v[e]);
  *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(tmp);
}

// acc[0] += scale * sum |a - b|.  loss_kernel's shape: 16-byte loads, fp32 partial sums, wave and workgroup reduction, one atomicAdd
// per workgroup.  A thread keeps one accumulator per component of its load (V = 4 or 8 independent chains of
// ceil(nvec / (grid * 256)) terms each) and folds them pairwise; the first nvec * V elements go through the vector loop (nvec = 0
// when a pointer is not 16-byte aligned), the rest through the scalar one.
template <typename T>
__global__ __launch_bounds__(256) void fm_l1_kernel(const T* __restrict__ a, const T* __restrict__ b, long n, long nvec, float scale,
                                                    float* __restrict__ acc) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ float red[32];
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  float s[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[e] = 0.f;
  for (long i = tid; i < nvec; i += stride) {
    float av[V], bv[V];
    ld16<T>(a + i * V, av);
    ld16<T>(b + i * V, bv);
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] += fabsf(av[e] - bv[e]);
  }
#pragma unroll
  for (int w = V / 2; w > 0; w >>= 1)
#pragma unroll
    for (int e = 0; e < w; ++e) s[e] += s[e + w];
  float t = s[0];
  for (long i = nvec * V + tid; i < n; i += stride) t += fabsf(ld<T>(a + i) - ld<T>(b + i));
  t = block_sum(t, red);
  if (threadIdx.x == 0) atomicAdd(acc, t * scale);
}

// g += c * sign(af - ar) * LeakyReLU'(af), c = coef * upstream[0]: the gradient of c * sum |af - ar| with respect to the
// PRE-activation of af, added to the gradient the data-gradient conv left there.  LeakyReLU'(af) = (af >= 0 ? 1 : slope), the
// convention of that conv's epilogue (disc_fused.hip: `svals[e] >= 0.f ? g : g * slope`); sign(0) = 0 as in F.l1_loss.  fp32
// arithmetic with one rounding to T: the two possible magnitudes c and c * slope are formed once (__fmul_rn: never contracted into
// the add), so an element is g, g + m or g - m.
template <typename T>
__global__ __launch_bounds__(256) void fm_inject_kernel(T* __restrict__ g, const T* __restrict__ af, const T* __restrict__ ar, long n,
                                                        long nvec, const float* __restrict__ upstream, float coef, float slope) {
  constexpr int V = 16 / (int)sizeof(T);
  const float c = __fmul_rn(coef, upstream[0]), cs = __fmul_rn(c, slope);
  auto one = [&](float gv, float f, float r) {
    const float m = f >= 0.f ? c : cs;
    return f > r ? gv + m : (f < r ? gv - m : gv);
  };
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < nvec; i += stride) {
    float gv[V], fv[V], rv[V];
    ld16<T>(g + i * V, gv);
    ld16<T>(af + i * V, fv);
    ld16<T>(ar + i * V, rv);
#pragma unroll
    for (int e = 0; e < V; ++e) gv[e] = one(gv[e], fv[e], rv[e]);
    st16<T>(g + i * V, gv);
  }
  for (long i = nvec * V + tid; i < n; i += stride) st<T>(g + i, one(ld<T>(g + i), ld<T>(af + i), ld<T>(ar + i)));
}

// ------------------------------------------------------------------------------------------- AdamW on a flat fp32 arena
// one element of torch.optim.AdamW: decoupled weight decay, the two moments, the bias-corrected step
__device__ __forceinline__ void adamw_update(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd,
                                             float bc1, float bc2, float gscale) {
  const float gr = g * gscale;
  float pi = p * (1.f - lr * wd);                      // decoupled weight decay (torch.optim.AdamW)
  const float mi = b1 * m + (1.f - b1) * gr;
  const float vi = b2 * v + (1.f - b2) * gr * gr;
  m = mi; v = vi;
  const float denom = sqrtf(vi) / sqrtf(bc2) + eps;
  pi -= (lr / bc1) * (mi / denom);
  p = pi;
}

// The one AdamW kernel.  Every per-step input comes either by value or from device memory, each device pointer optional:
//   hp   {lr, beta1, beta2, eps, weight_decay} (fp32) - the host refreshes them before each replay of a captured step, so schedules,
//        lr changes and restored counts reach the graph; NULL: the by-value arguments
//   step the step count (int32, already incremented: a captured HIP graph must not bake the host's count into its launch arguments),
//        the bias corrections are then formed here; NULL: bc1 / bc2 as the host formed them
//   coef the clip coefficient (the device slot grad_norm_finish_kernel wrote): g is multiplied by gscale * coef[0]; NULL: by gscale
//        alone.  gscale * 1.0f is gscale, so with a coefficient of exactly 1 the update has the bits of the unclipped form.
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, const float* __restrict__ hp,
                                                    const int* __restrict__ step, float lr, float b1, float b2, float eps, float wd,
                                                    float bc1, float bc2, float gscale_, const float* __restrict__ coef) {
  if (hp) { lr = hp[0]; b1 = hp[1]; b2 = hp[2]; eps = hp[3]; wd = hp[4]; }
  if (step) {
    const float t = (float)(*step);
    bc1 = 1.f - powf(b1, t); bc2 = 1.f - powf(b2, t);
  }
  const float gscale = coef ? gscale_ * coef[0] : gscale_;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    adamw_update(p[i], g[i], m[i], v[i], lr, b1, b2, eps, wd, bc1, bc2, gscale);
}

// ------------------------------------------------------------------------------------------- weight EMA on the arena
// Two streaming kernels over fp32 buffers of any length behind any 4-byte-aligned pointers (optim.ArenaEMA: the generator arena and
// its average).  The host splits [0, n) into a scalar head of `head` elements (up to the first 16-byte boundary), `nvec` 16-byte
// groups and a scalar tail; a work item below nvec is one group, item nvec + j is the j-th scalar element (head first, then tail).
// nvec = 0 when the two pointers are not congruent modulo 16 bytes.  Plain vector loads and stores, no LDS, no atomics.
__device__ __forceinline__ long ema_scalar_index(long j, long head, long nvec) { return j < head ? j : j + 4 * nvec; }

// ema[i] = fmaf(w, p[i] - ema[i], ema[i]): a subtraction, then ONE fused multiply-add (two roundings per update; the tests' error
// bound is derived from exactly this expression).  w = 1 - decay: *omd_dev when given - a captured step reads it from device memory
// at every replay - otherwise the argument.
__device__ __forceinline__ float ema_one(float e, float p, float w) { return fmaf(w, __fsub_rn(p, e), e); }

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, long head,
                                                         long nvec, const float* __restrict__ omd_dev, float omd) {
  const float w = omd_dev ? omd_dev[0] : omd;
  const long items = nvec + (n - 4 * nvec), stride = (long)gridDim.x * blockDim.x;
  float4* e4 = reinterpret_cast<float4*>(ema + head);
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
    if (i < nvec) {
      float4 e = e4[i];
      const float4 v = p4[i];
      e.x = ema_one(e.x, v.x, w); e.y = ema_one(e.y, v.y, w); e.z = ema_one(e.z, v.z, w); e.w = ema_one(e.w, v.w, w);
      e4[i] = e;
    } else {
      const long k = ema_scalar_index(i - nvec, head, nvec);
      ema[k] = ema_one(ema[k], p[k], w);
    }
  }
}

// a[i] <-> b[i] (the ranges do not overlap: refused by the entry point)
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n, long head, long nvec) {
  const long items = nvec + (n - 4 * nvec), stride = (long)gridDim.x * blockDim.x;
  float4* a4 = reinterpret_cast<float4*>(a + head);
  float4* b4 = reinterpret_cast<float4*>(b + head);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += stride) {
    if (i < nvec) {
      const float4 x = a4[i], y = b4[i];
      a4[i] = y; b4[i] = x;
    } else {
      const long k = ema_scalar_index(i - nvec, head, nvec);
      const float x = a[k], y = b[k];
      a[k] = y; b[k] = x;
    }
  }
}

// gather many gradient tensors (any storage type, given per tensor) into one flat fp32 buffer: flat[dst_off + i] = src[i], a NULL
// source writes zeros.  ACC, the accumulating form (gradient accumulation: micro-steps 2..N of a window): flat[dst_off + i] += src[i],
// one fp32 add per element; a NULL source adds nothing (the block returns before touching memory).  Neither form touches the padding
// words between parameters, which therefore stay zero from the arena's allocation on (grad_norm_partial_kernel reads them as part
// of its slice).
struct GatherDesc { const void* src; long dst_off; long n; int dtype; int pad; };
template <bool ACC>
__global__ __launch_bounds__(256) void multi_gather_kernel(const GatherDesc* __restrict__ descs, float* __restrict__ flat, int chunk) {
  const GatherDesc d = descs[blockIdx.y];
  const long beg = (long)blockIdx.x * chunk;
  if ((ACC && d.src == nullptr) || beg >= d.n) return;
  const long end = beg + chunk < d.n ? beg + chunk : d.n;
  for (long i = beg + threadIdx.x; i < end; i += blockDim.x) {
    float v;
    if (d.src == nullptr) v = 0.f;
    else if (d.dtype == MV_F32) v = ((const float*)d.src)[i];
    else if (d.dtype == MV_BF16) v = ld<bf16>((const bf16*)d.src + i);
    else v = ld<f16>((const f16*)d.src + i);
    if (ACC) flat[d.dst_off + i] += v;
    else flat[d.dst_off + i] = v;
  }
}

// ------------------------------------------------------------------------------------------- gradient norm + clip coefficient
// torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False) over one fp32 arena slice, in two launches and without
// floating-point atomics, so the same input gives the same bits on every run:
//   stage 1: a FIXED grid of GN_GRID workgroups x 256 threads, grid-stride over 16-byte groups; one double partial per workgroup
//   stage 2: one workgroup adds the GN_GRID partials in a fixed order (double) and writes
//            out[0] = norm = |pre_scale| * sqrt(sum g^2),  out[1] = coef = min(1, max_norm / (norm + 1e-6))   (fp32, torch's formula)
// Longest chain of dependent fp32 additions: GN_FLUSH + 2 = 34.  A thread squares into four independent fp32 accumulators (one per
// component of its 16-byte load: a chain of at most GN_FLUSH = 32 adds each), folds them with two more adds and moves the result into
// a double; everything behind that - the rest of the thread's sweep, the wave butterfly, the cross-wave and cross-workgroup sums -
// is double, at any arena length.  All terms are non-negative, so the fp32 part's relative error is at most 34 * 2^-24 = 2e-6.
constexpr int GN_GRID = 1024, GN_FLUSH = 32;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partials) {
  __shared__ double red[4];
  const long n4 = n >> 2, stride = (long)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double acc = 0.0;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  while (i < n4) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < GN_FLUSH && i < n4; ++k, i += stride) {
      const float4 v = g4[i];
      a0 += v.x * v.x; a1 += v.y * v.y; a2 += v.z * v.z; a3 += v.w * v.w;
    }
    acc += (double)((a0 + a1) + (a2 + a3));
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {      // a slice length that is no multiple of 4 (the arena's own is one of 8)
    const float v = g[(n4 << 2) + threadIdx.x];
    acc += (double)(v * v);
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, int n_partials, float pre_scale,
                                                               const float* __restrict__ max_norm_dev, float max_norm,
                                                               float* __restrict__ out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x) acc += partials[i];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = (red[0] + red[1]) + (red[2] + red[3]);
    const float norm = (float)(fabs((double)pre_scale) * sqrt(sum));
    const float mx = max_norm_dev ? max_norm_dev[0] : max_norm;
    const float c = mx / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;          // (a NaN norm stays a NaN coefficient, an infinite one gives 0: torch.clamp(max=1))
  }
}

// ------------------------------------------------------------------------------------------- log-mel spectrogram loss
// frames: reflect-pad (n_fft-hop)/2, hop, periodic Hann; |rFFT| (power-of-two n_fft: radix-2 FFT of the frame in LDS, forward and
// adjoint; otherwise a direct O(N^2) DFT with an exact (k*n mod N) twiddle table), mel = fb @ mag, logmel = log(max(mel, clamp)); loss = weight * mean |logmel - target|.
// One workgroup per (b, frame).  Backward recomputes the frame spectrum and scatters d wave with atomics (frames overlap 4x).
__device__ __forceinline__ int reflect_idx(int i, int Tn) {
  if (i < 0) i = -i;
  if (i >= Tn) i = 2 * (Tn - 1) - i;
  return i;
}

// In-LDS radix-2 FFT of N = 2^logn complex points (decimation in time; the caller stored its input in bit-reversed order).
// sgn = -1: forward transform e^{-2 pi i kn/N}; +1: the adjoint.  Twiddles come from the shared cos/sin tables (index j*N/m),
// N/2 butterflies per stage spread over the workgroup, one barrier per stage.
__device__ __forceinline__ void lds_fft(float* xr, float* xi, const float* ct, const float* stb, int logn, float sgn) {
  const int N = 1 << logn;
  for (int s = 1; s <= logn; ++s) {
    const int half = 1 << (s - 1), tws = N >> s;
    for (int j = threadIdx.x; j < N / 2; j += blockDim.x) {
      const int pos = j & (half - 1), i0 = ((j >> (s - 1)) << s) + pos, i1 = i0 + half;
      const float wr = ct[pos * tws], wi = sgn * stb[pos * tws];
      const float ar = xr[i1], ai = xi[i1];
      const float tr = wr * ar - wi * ai, ti = wr * ai + wi * ar;
      const float br = xr[i0], bi = xi[i0];
      xr[i1] = br - tr; xi[i1] = bi - ti;
      xr[i0] = br + tr; xi[i0] = bi + ti;
    }
    __syncthreads();
  }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void mel_loss_kernel(const T* __restrict__ wave, const float* __restrict__ fb,
                                                       const float* __restrict__ target, float* __restrict__ mel_out,
                                                       float* __restrict__ loss_acc, float* __restrict__ gwave,
                                                       int Tn, int n_fft, int hop, int n_mels, int n_frames, float clampv,
                                                       float weight, long n_total, int kind, int logn) {
  extern __shared__ float sm[];
  const int nb = n_fft / 2 + 1;
  // logn > 0 (n_fft a power of two): rFFT path - re / im hold all n_fft points of the in-LDS FFT, `scr` the adjoint's imaginary part
  float* fr = sm;                 // [n_fft] windowed frame
  float* ct = fr + n_fft;         // [n_fft] cos table
  float* stb = ct + n_fft;        // [n_fft] sin table
  float* re = stb + n_fft;        // [nb], FFT: [n_fft]
  float* im = re + (logn > 0 ? n_fft : nb);
  float* scr = im + (logn > 0 ? n_fft : nb);   // FFT: [n_fft]
  float* mag = scr + (logn > 0 ? n_fft : 0);   // [nb]
  float* gml = mag + nb;          // [n_mels] dL/dmel
  float* red = gml + n_mels;      // [32]
  const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
  const int padn = (n_fft - hop) / 2;
  const float w0 = 6.283185307179586f / (float)n_fft;
  for (int n = tid; n < n_fft; n += blockDim.x) {
    const float win = 0.5f - 0.5f * cosf(w0 * n);
    const int ti = reflect_idx(f * hop - padn + n, Tn);
    fr[n] = ld<T>(wave + (long)b * Tn + ti) * win;
    ct[n] = cosf(w0 * n);
    stb[n] = sinf(w0 * n);
  }
  __syncthreads();
  if (logn > 0) {
    for (int n = tid; n < n_fft; n += blockDim.x) {
      const int r = (int)(__brev((unsigned)n) >> (32 - logn));
      re[r] = fr[n]; im[r] = 0.f;
    }
    __syncthreads();
    lds_fft(re, im, ct, stb, logn, -1.f);
    for (int k = tid; k < nb; k += blockDim.x) mag[k] = sqrtf(re[k] * re[k] + im[k] * im[k] + 1e-9f);
  } else {
    for (int k = tid; k < nb; k += blockDim.x) {
      float a = 0.f, c = 0.f;
      int idx = 0;
      for (int n = 0; n < n_fft; ++n) {
        a += fr[n] * ct[idx];
        c -= fr[n] * stb[idx];
        idx += k; if (idx >= n_fft) idx -= n_fft;
      }
      re[k] = a; im[k] = c;
      mag[k] = sqrtf(a * a + c * c + 1e-9f);
    }
  }
  __syncthreads();
  float lsum = 0.f;
  for (int m = tid; m < n_mels; m += blockDim.x) {
    float a = 0.f;
    for (int k = 0; k < nb; ++k) a += fb[(long)m * nb + k] * mag[k];
    const float lm = logf(fmaxf(a, clampv));
    if (mel_out) mel_out[((long)b * n_mels + m) * n_frames + f] = lm;
    float g = 0.f;
    if (target) {
      const float d = lm - target[((long)b * n_mels + m) * n_frames + f];
      lsum += kind == 0 ? fabsf(d) : d * d;
      g = (kind == 0 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d) * (weight / (float)n_total);
    }
    gml[m] = (a > clampv) ? g / a : 0.f;       // d/d mel through log(clamp)
  }
  if (loss_acc && target) {
    lsum = block_sum(lsum, red);
    if (tid == 0) atomicAdd(loss_acc, lsum * weight / (float)n_total);
  }
  if (!BWD) return;
  __syncthreads();
  // g_mag[k] = sum_m fb[m][k] gml[m] ; g_re = g_mag re/mag ; g_im = g_mag im/mag
  for (int k = tid; k < nb; k += blockDim.x) {
    float a = 0.f;
    for (int m = 0; m < n_mels; ++m) a += fb[(long)m * nb + k] * gml[m];
    const float inv = a / mag[k];
    re[k] *= inv; im[k] *= inv;    // now g_re, g_im
  }
  __syncthreads();
  // g_frame[n] = sum_k g_re cos(2 pi k n/N) - g_im sin(2 pi k n/N) ; d wave += g_frame * win
  if (logn > 0) {
    // = Re( sum_{k < nb} (g_re + i g_im) e^{+2 pi i kn/N} ): the adjoint FFT of the half spectrum, zero above Nyquist
    for (int k = tid; k < n_fft; k += blockDim.x) {
      const int r = (int)(__brev((unsigned)k) >> (32 - logn));
      fr[r] = k < nb ? re[k] : 0.f; scr[r] = k < nb ? im[k] : 0.f;
    }
    __syncthreads();
    lds_fft(fr, scr, ct, stb, logn, 1.f);
  }
  for (int n = tid; n < n_fft; n += blockDim.x) {
    float a = 0.f;
    if (logn > 0) a = fr[n];
    else {
      int idx = 0;
      for (int k = 0; k < nb; ++k) {
        a += re[k] * ct[idx] - im[k] * stb[idx];
        idx += n; if (idx >= n_fft) idx -= n_fft;
      }
    }
    const float win = 0.5f - 0.5f * ct[n];
    const int ti = reflect_idx(f * hop - padn + n, Tn);
    atomicAdd(gwave + (long)b * Tn + ti, a * win);
  }
}

}  // namespace mv

using namespace mv;

static inline int grid_for(long n, int block = 256, int cap = 2048) {
  long g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" int mv_dropout_mask(uint8_t* mask, long n, float p, long seed_, void* stream) {
  const uint64_t seed = (uint64_t)seed_;
  MV_CHECK_ARG(mask && n > 0 && p >= 0.f && p < 1.f && ((uintptr_t)mask & 7) == 0);
  const uint32_t thresh = (uint32_t)(p * 65536.f + 0.5f);
  const long nblk = (n + 7) / 8;
  const unsigned grid = (unsigned)((nblk + 255) / 256 > 4096 ? 4096 : (nblk + 255) / 256);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mask, n, thresh, (uint32_t)seed, (uint32_t)(seed >> 32));
  MV_LAUNCH_CHECK();
  return MV_OK;
}

static inline unsigned dropout_grid(long n) {
  const long nblk = (n + 7) / 8;
  return (unsigned)((nblk + 255) / 256 > 4096 ? 4096 : (nblk + 255) / 256);
}

extern "C" int mv_dropout_mask_ctr(uint8_t* mask, long n, float p, long key, long ctr, void* stream) {
  MV_CHECK_ARG(mask && n > 0 && p >= 0.f && p < 1.f && ((uintptr_t)mask & 7) == 0);
  const uint32_t thresh = (uint32_t)(p * 65536.f + 0.5f);
  hipLaunchKernelGGL(dropout_mask_ctr_kernel, dim3(dropout_grid(n)), dim3(256), 0, (hipStream_t)stream, mask, n, thresh,
                     (const long long*)nullptr, (uint64_t)key, (uint64_t)ctr);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_dropout_mask_dev(uint8_t* mask, long n, float p, const long* state_dev, long slot, void* stream) {
  MV_CHECK_ARG(mask && state_dev && n > 0 && p >= 0.f && p < 1.f && ((uintptr_t)mask & 7) == 0 && ((uintptr_t)state_dev & 7) == 0);
  const uint32_t thresh = (uint32_t)(p * 65536.f + 0.5f);
  hipLaunchKernelGGL(dropout_mask_ctr_kernel, dim3(dropout_grid(n)), dim3(256), 0, (hipStream_t)stream, mask, n, thresh,
                     (const long long*)state_dev, (uint64_t)0, (uint64_t)slot);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_grc_fold_bwd(const float* g_weff, const float* g_beff, const void* conv_w, const void* conv_b,
                               const void* lora_A, const void* lora_B, const void* lora_scaling, const void* proj_w,
                               float* g_conv_w, float* g_conv_b, float* g_A, float* g_B, float* g_s, float* g_proj_w,
                               float* g_proj_b, int Cin, int Cout, int ks, int groups, int rank, int param_dtype,
                               void* stream) {
  MV_CHECK_ARG(g_weff && g_beff && conv_w && conv_b && lora_A && lora_B && lora_scaling && proj_w);
  MV_CHECK_ARG(g_conv_w && g_conv_b && g_A && g_B && g_s && g_proj_w && g_proj_b && (ks & 1) && Cin % groups == 0 && Cout % groups == 0);
  const size_t lds = sizeof(float) * (2 * (size_t)Cout * Cin * ks + (size_t)Cin * Cout + 32 + (size_t)Cout * (Cin / groups) * ks +
                                      (size_t)Cout * Cout + (size_t)Cin * rank + (size_t)rank * Cout);
  if (lds > 160 * 1024) return MV_ERR_UNSUPPORTED;
#define GO(P) { auto kern = grc_fold_bwd_kernel<P>; \
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), lds, (hipStream_t)stream, g_weff, g_beff, (const P*)conv_w, (const P*)conv_b, \
      (const P*)lora_A, (const P*)lora_B, (const P*)lora_scaling, (const P*)proj_w, g_conv_w, g_conv_b, g_A, g_B, g_s, g_proj_w, \
      g_proj_b, Cin, Cout, ks, groups, rank); }
  switch (param_dtype) {
    case MV_F32: GO(float); break;
    case MV_BF16: GO(bf16); break;
    case MV_F16: GO(f16); break;
    default: return MV_ERR_DTYPE;
  }
#undef GO
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_loss_fwd_bwd(const void* x, const void* y, float c, float weight, float* loss_acc, void* gx, void* gy,
                               long n, int kind, int dtype, void* stream) {
  MV_CHECK_ARG(x && loss_acc && n > 0 && kind >= 0 && kind <= 4 && ((kind != 1 && kind != 4) || y));
  MV_DISPATCH(dtype, hipLaunchKernelGGL(loss_kernel<T>, dim3(grid_for(n, 256, 512)), dim3(256), 0, (hipStream_t)stream,
                                        (const T*)x, (const T*)y, c, weight, loss_acc, (T*)gx, (T*)gy, n, kind));
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_scale(void* x, const float* factor_dev, float factor, long n, int dtype, void* stream) {
  MV_CHECK_ARG(x && n > 0);
  MV_DISPATCH(dtype, hipLaunchKernelGGL(scale_kernel<T>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (T*)x,
                                        factor_dev, factor, n));
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_scale_to(const void* x, void* y, const float* factor_dev, float factor, long n, int dtype, void* stream) {
  MV_CHECK_ARG(x && y && n > 0);
  MV_DISPATCH(dtype, hipLaunchKernelGGL(scale_to_kernel<T>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y,
                                        factor_dev, factor, n));
  MV_LAUNCH_CHECK();
  return MV_OK;
}

// elements of T that go through 16-byte accesses: all whole groups when every pointer is 16-byte aligned, none otherwise
template <typename T> static long fm_nvec(long n, const void* a, const void* b, const void* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) ? 0 : n / (16 / (long)sizeof(T));
}

extern "C" int mv_fm_l1(const void* a, const void* b, long n, float scale, float* acc, int dtype, void* stream) {
  MV_CHECK_ARG(a && b && acc && n > 0);
  // at most 1024 workgroups: the atomics on acc form a chain of that many fp32 additions at the most
  MV_DISPATCH(dtype, {
    const long nvec = fm_nvec<T>(n, a, b, nullptr);
    hipLaunchKernelGGL(fm_l1_kernel<T>, dim3(grid_for(nvec ? nvec : n, 256, 1024)), dim3(256), 0, (hipStream_t)stream, (const T*)a,
                       (const T*)b, n, nvec, scale, acc);
  });
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_fm_inject(void* g, const void* af, const void* ar, long n, const float* upstream_dev, float coef, float slope,
                            int dtype, void* stream) {
  MV_CHECK_ARG(g && af && ar && upstream_dev && n > 0 && g != af && g != ar);
  MV_DISPATCH(dtype, {
    const long nvec = fm_nvec<T>(n, g, af, ar);
    hipLaunchKernelGGL(fm_inject_kernel<T>, dim3(grid_for(nvec ? nvec : n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, (T*)g,
                       (const T*)af, (const T*)ar, n, nvec, upstream_dev, coef, slope);
  });
  MV_LAUNCH_CHECK();
  return MV_OK;
}

// The one AdamW launch.  step_dev NULL: the bias corrections are formed here from `step`, like torch's host-side ones.
static int adamw_launch(float* p, const float* g, float* m, float* v, long n, const float* hparams_dev, const int* step_dev, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, const float* coef_dev,
                        void* stream) {
  float bc1 = 1.f, bc2 = 1.f;
  if (!step_dev) { bc1 = 1.f - powf(beta1, (float)step); bc2 = 1.f - powf(beta2, (float)step); }
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, hparams_dev,
                     step_dev, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, coef_dev);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_adamw_flat(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, float grad_scale, void* stream) {
  MV_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
  return adamw_launch(p, g, m, v, n, nullptr, nullptr, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}

extern "C" int mv_adamw_flat_dev(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, const int* step_dev, float grad_scale, void* stream) {
  MV_CHECK_ARG(p && g && m && v && n > 0 && step_dev);
  return adamw_launch(p, g, m, v, n, nullptr, step_dev, lr, beta1, beta2, eps, weight_decay, 0, grad_scale, nullptr, stream);
}

extern "C" int mv_adamw_flat_hp(float* p, const float* g, float* m, float* v, long n, const float* hparams_dev, const int* step_dev,
                                float grad_scale, void* stream) {
  MV_CHECK_ARG(p && g && m && v && n > 0 && hparams_dev && step_dev);
  return adamw_launch(p, g, m, v, n, hparams_dev, step_dev, 0.f, 0.f, 0.f, 0.f, 0.f, 0, grad_scale, nullptr, stream);
}

extern "C" int mv_adamw_flat_clip(float* p, const float* g, float* m, float* v, long n, const float* hparams_dev, const int* step_dev,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                  const float* coef_dev, void* stream) {
  MV_CHECK_ARG(p && g && m && v && n > 0 && coef_dev && (step_dev || step >= 1));
  return adamw_launch(p, g, m, v, n, hparams_dev, step_dev, lr, beta1, beta2, eps, weight_decay, step, grad_scale, coef_dev, stream);
}

// The head / body / tail split of ema_update_kernel and swap_kernel: 16-byte groups only when a and b reach a 16-byte boundary at the
// same element (arena buffers always do, at element 0).
struct PairSplit { long head, nvec; };
static PairSplit pair_split(const float* a, const float* b, long n) {
  if ((((uintptr_t)a ^ (uintptr_t)b) & 15) != 0) return {0, 0};
  long head = (long)(((16 - ((uintptr_t)a & 15)) & 15) / sizeof(float));
  if (head > n) head = n;
  return {head, (n - head) / 4};
}
static bool ranges_overlap(const float* a, const float* b, long n) {
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return ua < ub + len && ub < ua + len;
}

extern "C" int mv_ema_update(float* ema, const float* p, long n, const float* omd_dev, float omd, void* stream) {
  MV_CHECK_ARG(n >= 0);
  if (n == 0) return MV_OK;            // (an empty range has no address to speak of)
  MV_CHECK_ARG(ema && p && (((uintptr_t)ema | (uintptr_t)p | (uintptr_t)omd_dev) & 3) == 0 && !ranges_overlap(ema, p, n));
  const PairSplit s = pair_split(ema, p, n);
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(s.nvec + (n - 4 * s.nvec), 256, 4096)), dim3(256), 0, (hipStream_t)stream, ema, p,
                     n, s.head, s.nvec, omd_dev, omd);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_swap_f32(float* a, float* b, long n, void* stream) {
  MV_CHECK_ARG(n >= 0);
  if (n == 0) return MV_OK;
  MV_CHECK_ARG(a && b && (((uintptr_t)a | (uintptr_t)b) & 3) == 0 && !ranges_overlap(a, b, n));
  const PairSplit s = pair_split(a, b, n);
  hipLaunchKernelGGL(swap_kernel, dim3(grid_for(s.nvec + (n - 4 * s.nvec), 256, 4096)), dim3(256), 0, (hipStream_t)stream, a, b, n,
                     s.head, s.nvec);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

template <bool ACC>
static int gather_launch(const void* descs_dev, int n_tensors, long max_len, float* flat, void* stream) {
  MV_CHECK_ARG(descs_dev && flat && n_tensors > 0 && n_tensors <= 65535 && max_len > 0);
  const int chunk = 16384;
  dim3 grid((unsigned)((max_len + chunk - 1) / chunk), n_tensors);
  hipLaunchKernelGGL(multi_gather_kernel<ACC>, grid, dim3(256), 0, (hipStream_t)stream, (const GatherDesc*)descs_dev, flat, chunk);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_multi_gather(const void* descs_dev, int n_tensors, long max_len, float* flat, void* stream) {
  return gather_launch<false>(descs_dev, n_tensors, max_len, flat, stream);
}

extern "C" int mv_multi_gather_acc(const void* descs_dev, int n_tensors, long max_len, float* flat, void* stream) {
  return gather_launch<true>(descs_dev, n_tensors, max_len, flat, stream);
}

extern "C" int mv_zero_f32(float* x, long n, void* stream) {
  MV_CHECK_ARG(x && n > 0 && ((uintptr_t)x & 15) == 0);      // 16-byte aligned: always the fill kernel, never a memset node
  MV_HIP(mvi_zero_async(x, sizeof(float) * (size_t)n, (hipStream_t)stream));
  return MV_OK;
}

static_assert(sizeof(double) * GN_GRID == MV_GRAD_NORM_WORKSPACE_BYTES, "header and kernel disagree on the partials' size");

extern "C" int mv_grad_norm(const float* g, long n, float pre_scale, const float* max_norm_dev, float max_norm, void* workspace,
                            float* out, void* stream) {
  MV_CHECK_ARG(g && workspace && out && n > 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
  MV_CHECK_ARG(max_norm_dev || max_norm > 0.f);
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(GN_GRID), dim3(256), 0, (hipStream_t)stream, g, n, (double*)workspace);
  MV_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, GN_GRID, pre_scale,
                     max_norm_dev, max_norm, out);
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_mel_loss(const void* wave, const float* fb, const float* target, float* mel_out, float* loss_acc,
                           float* gwave, int B, int T_, int n_fft, int hop, int n_mels, float clampv, float weight,
                           int kind, int backward, int dtype, void* stream) {
  MV_CHECK_ARG(wave && fb && B > 0 && T_ > 0 && n_fft > 0 && hop > 0 && n_mels > 0 && T_ % hop == 0 && n_fft >= hop);
  MV_CHECK_ARG(!backward || (gwave && target));
  MV_CHECK_ARG(kind == 0 || kind == 1);
  MV_CHECK_ARG((n_fft - hop) / 2 < T_);
  const int n_frames = T_ / hop, nb = n_fft / 2 + 1;
  int logn = 0;                                       // rFFT path for power-of-two n_fft, the direct DFT otherwise
  if (n_fft >= 32 && (n_fft & (n_fft - 1)) == 0) while ((1 << logn) < n_fft) ++logn;
  const size_t lds = sizeof(float) * ((logn > 0 ? 6 * (size_t)n_fft + nb : 3 * (size_t)n_fft + 3 * (size_t)nb) + n_mels + 32);
  if (lds > 160 * 1024 || B > 65535) return MV_ERR_UNSUPPORTED;
  const long n_total = (long)B * n_mels * n_frames;
  dim3 grid(n_frames, B);
  MV_DISPATCH(dtype, {
    if (backward) {
      auto kern = mel_loss_kernel<T, true>;
      if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, (const T*)wave, fb, target, mel_out,
                         loss_acc, gwave, T_, n_fft, hop, n_mels, n_frames, clampv, weight, n_total, kind, logn);
    } else {
      auto kern = mel_loss_kernel<T, false>;
      if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, (const T*)wave, fb, target, mel_out,
                         loss_acc, gwave, T_, n_fft, hop, n_mels, n_frames, clampv, weight, n_total, kind, logn);
    }
  });
  MV_LAUNCH_CHECK();
  return MV_OK;
}
