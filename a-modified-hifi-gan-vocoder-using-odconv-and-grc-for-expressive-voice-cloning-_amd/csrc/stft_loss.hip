// Multi-resolution STFT loss (spectral convergence + log-magnitude L1, after Yamamoto et al. 2020); defined by this build
// (include/mi355x_vocoder.h: mv_stft_loss).  The framing is the mel kernel's (train.hip): reflect pad (n_fft-hop)/2,
// frame f starts at f*hop - pad, periodic Hann.
//
// One workgroup per (resolution, b, frame), every resolution in one launch per pass.  The windowed REAL frame is the real part and
// the windowed FAKE frame the imaginary part of ONE complex in-LDS radix-2 FFT ("two for one"); with Z its result
//   X_real[k] = (Z[k] + conj Z[N-k]) / 2        X_fake[k] = (Z[k] - conj Z[N-k]) / (2i)         k = 0 .. N/2
// LDS: Z as interleaved (re, im) pairs (8 N bytes: one 8-byte access per point) + N/2 twiddle pairs (4 N bytes) + 128 bytes for the
// workgroup sums: 24.1 KB at n_fft 2048, sized by the launch's largest n_fft.
//   forward: decimation in time, the load writes the frame in bit-reversed order, the spectrum comes out in natural order
//   adjoint: decimation in frequency on the spectrum where it lies, the frame gradient comes out in bit-reversed order
// so neither direction needs a permutation pass, and the thread that owns bins k and N-k turns them into g_X[k] and 0 in place.
//
// An exact zero: the butterflies are written with explicit fmaf / __fmul_rn and the twiddle table is mirrored about N/4 (entry N/2-j
// is (-cos_j, sin_j) bit for bit).  Exchanging the two inputs then exchanges re and im of bin k with those of bin N-k bit for bit
// (induction over the stages), so fake == real gives X_fake == X_real in every bit, S_num = 0, and loss and gradient are exactly 0.
#include "common.h"

namespace mv {

constexpr int STFT_MAX_RES = 8;
constexpr int STFT_MIN_NFFT = 32, STFT_MAX_NFFT = 2048;

struct StftRes {
  int n_fft, hop, logn, n_frames;
  int first_block;      // of this resolution's B * n_frames workgroups
  float inv_n;          // 1 / (B * (n_fft/2+1) * n_frames)
};
struct StftPlan {
  StftRes res[STFT_MAX_RES];
  int n_res, B, Tn;
  float floorv, scale;  // scale = weight / n_res
};

__device__ __forceinline__ int stft_reflect(int i, int Tn) {
  if (i < 0) i = -i;
  if (i >= Tn) i = 2 * (Tn - 1) - i;
  return i;
}

// (w.x, w.y) * (a.x, a.y) with a fixed rounding pattern: the second product is rounded, the first one fused.  Negating w.x, or
// exchanging a.x and a.y together with the sign of w.y, changes the results by the same signs / exchange and by nothing else.
__device__ __forceinline__ float2 stft_cmul(float2 w, float2 a) {
  return make_float2(fmaf(w.x, a.x, -__fmul_rn(w.y, a.y)), fmaf(w.x, a.y, __fmul_rn(w.y, a.x)));
}

// Forward transform e^{-2 pi i kn/N} of z (bit-reversed on entry, natural order on exit).  N/2 butterflies per stage over the
// workgroup, one barrier per stage; tw[j] = (cos, sin)(2 pi j / N).
__device__ __forceinline__ void stft_fft_dit(float2* z, const float2* tw, int logn) {
  const int N = 1 << logn;
  for (int s = 1; s <= logn; ++s) {
    const int half = 1 << (s - 1), tws = N >> s;
    for (int j = threadIdx.x; j < N / 2; j += blockDim.x) {
      const int pos = j & (half - 1), i0 = ((j >> (s - 1)) << s) + pos, i1 = i0 + half;
      const float2 c = tw[pos * tws];
      const float2 t = stft_cmul(make_float2(c.x, -c.y), z[i1]), a = z[i0];
      z[i1] = make_float2(a.x - t.x, a.y - t.y);
      z[i0] = make_float2(a.x + t.x, a.y + t.y);
    }
    __syncthreads();
  }
}

// Adjoint transform e^{+2 pi i kn/N} of z (natural order on entry, bit-reversed on exit).
__device__ __forceinline__ void stft_fft_dif_adj(float2* z, const float2* tw, int logn) {
  const int N = 1 << logn;
  for (int s = logn; s >= 1; --s) {
    const int half = 1 << (s - 1), tws = N >> s;
    for (int j = threadIdx.x; j < N / 2; j += blockDim.x) {
      const int pos = j & (half - 1), i0 = ((j >> (s - 1)) << s) + pos, i1 = i0 + half;
      const float2 a = z[i0], b = z[i1];
      z[i0] = make_float2(a.x + b.x, a.y + b.y);
      z[i1] = stft_cmul(tw[pos * tws], make_float2(a.x - b.x, a.y - b.y));
    }
    __syncthreads();
  }
}

// BWD = false: sums[r] += {S_num, S_den, sum |log M_fake - log M_real|} of this frame.
// BWD = true:  gwave += d (scale * sum_r (sc_r + mag_r)) / d fake, the sums read from device memory.
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void stft_loss_kernel(const T* __restrict__ fake, const T* __restrict__ real, float* __restrict__ sums,
                                                        float* __restrict__ gwave, const StftPlan plan) {
  extern __shared__ float2 stft_sm[];
  int r = 0;
  while (r + 1 < plan.n_res && (int)blockIdx.x >= plan.res[r + 1].first_block) ++r;
  const StftRes R = plan.res[r];
  const int N = R.n_fft, logn = R.logn, Tn = plan.Tn, tid = threadIdx.x;
  const int local = (int)blockIdx.x - R.first_block, b = local / R.n_frames, f = local % R.n_frames;
  float2* z = stft_sm;                         // [N]
  float2* tw = z + N;                          // [N/2]
  float* red = reinterpret_cast<float*>(tw + N / 2);   // [32]
  const int start = f * R.hop - (N - R.hop) / 2;
  const float inv_half = 2.f / (float)N;
  // twiddles: j <= N/4 from sincospif (exact argument), the rest mirrored
  for (int j = tid; j < N / 2; j += blockDim.x) {
    const int jm = j <= N / 4 ? j : N / 2 - j;
    float sn, cs;
    sincospif((float)jm * inv_half, &sn, &cs);
    if (jm == N / 4) { cs = 0.f; sn = 1.f; }
    tw[j] = make_float2(j <= N / 4 ? cs : -cs, sn);
  }
  const T* fk = fake + (long)b * Tn;
  const T* rl = real + (long)b * Tn;
  for (int n = tid; n < N; n += blockDim.x) {
    const float win = 0.5f - 0.5f * cospif((float)n * inv_half);
    const int ti = stft_reflect(start + n, Tn);
    z[__brev((unsigned)n) >> (32 - logn)] = make_float2(ld<T>(rl + ti) * win, ld<T>(fk + ti) * win);
  }
  __syncthreads();
  stft_fft_dit(z, tw, logn);
  const float fl = plan.floorv;
  float c_sc = 0.f, c_mag = 0.f;
  if (BWD) {
    const float s_num = sums[3 * r], s_den = sums[3 * r + 1];
    c_sc = s_num > 0.f ? plan.scale / (sqrtf(s_num) * sqrtf(s_den)) : 0.f;
    c_mag = plan.scale * R.inv_n;
  }
  float a_num = 0.f, a_den = 0.f, a_log = 0.f;
  for (int k = tid; k <= N / 2; k += blockDim.x) {
    const int km = (N - k) & (N - 1);
    const float2 p = z[k], q = z[km];
    const float xr_re = 0.5f * (p.x + q.x), xr_im = 0.5f * (p.y - q.y);     // X_real[k]
    const float xf_re = 0.5f * (p.y + q.y), xf_im = 0.5f * (q.x - p.x);     // X_fake[k]
    const float p_r = fmaxf(fmaf(xr_re, xr_re, __fmul_rn(xr_im, xr_im)), fl);
    const float p_f_raw = fmaf(xf_re, xf_re, __fmul_rn(xf_im, xf_im));
    const float p_f = fmaxf(p_f_raw, fl);
    const float m_r = sqrtf(p_r), m_f = sqrtf(p_f);
    if (!BWD) {
      const float d = m_r - m_f;
      a_num = fmaf(d, d, a_num);
      a_den += p_r;
      a_log += 0.5f * fabsf(logf(p_f) - logf(p_r));
    } else {
      float g = 0.f;
      if (p_f_raw > fl) {
        const float sg = p_f > p_r ? 1.f : (p_f < p_r ? -1.f : 0.f);
        g = (c_sc * (m_f - m_r) + c_mag * sg / m_f) / m_f;                  // g_M / M_f
      }
      z[k] = make_float2(g * xf_re, g * xf_im);                             // g_X[k]; this thread alone reads or writes k and N-k
      if (km > N / 2) z[km] = make_float2(0.f, 0.f);
    }
  }
  if (!BWD) {
    a_num = block_sum(a_num, red);
    a_den = block_sum(a_den, red);
    a_log = block_sum(a_log, red);
    if (tid == 0) {
      atomicAdd(sums + 3 * r, a_num);
      atomicAdd(sums + 3 * r + 1, a_den);
      atomicAdd(sums + 3 * r + 2, a_log);
    }
    return;
  }
  __syncthreads();
  stft_fft_dif_adj(z, tw, logn);
  float* gw = gwave + (long)b * Tn;
  for (int n = tid; n < N; n += blockDim.x) {
    const float win = 0.5f - 0.5f * cospif((float)n * inv_half);
    atomicAdd(gw + stft_reflect(start + n, Tn), z[__brev((unsigned)n) >> (32 - logn)].x * win);
  }
}

// loss[0] = scale * sum_r ( sqrt(S_num) / sqrt(S_den) + S_log / n_r )
__global__ __launch_bounds__(64) void stft_loss_finish_kernel(const float* __restrict__ sums, float* __restrict__ loss, const StftPlan plan) {
  if (threadIdx.x != 0) return;
  float acc = 0.f;
  for (int r = 0; r < plan.n_res; ++r)
    acc += sqrtf(sums[3 * r]) / sqrtf(sums[3 * r + 1]) + sums[3 * r + 2] * plan.res[r].inv_n;
  loss[0] = plan.scale * acc;
}

}  // namespace mv

using namespace mv;

extern "C" int mv_stft_loss(const void* fake, const void* real, int B, int T_, int n_res, const int* n_fft, const int* hop, float floorv,
                            float weight, float* sums, float* loss, float* gwave, int backward, int dtype, void* stream) {
  MV_CHECK_ARG(fake && real && n_fft && hop && sums && loss && B > 0 && T_ > 0 && n_res >= 1 && n_res <= STFT_MAX_RES);
  MV_CHECK_ARG(floorv > 0.f && (!backward || gwave));
  if (dtype != MV_F32 && dtype != MV_BF16 && dtype != MV_F16) return MV_ERR_DTYPE;      // (before the fill launch)
  StftPlan plan;
  plan.n_res = n_res; plan.B = B; plan.Tn = T_; plan.floorv = floorv; plan.scale = weight / (float)n_res;
  long blocks = 0;
  int max_fft = 0;
  for (int r = 0; r < n_res; ++r) {
    const int N = n_fft[r], h = hop[r];
    MV_CHECK_ARG(N >= STFT_MIN_NFFT && N <= STFT_MAX_NFFT && (N & (N - 1)) == 0);
    MV_CHECK_ARG(h >= 1 && h <= N && (N - h) % 2 == 0 && T_ % h == 0 && (N - h) / 2 < T_);
    StftRes& R = plan.res[r];
    R.n_fft = N; R.hop = h; R.n_frames = T_ / h; R.logn = 0;
    while ((1 << R.logn) < N) ++R.logn;
    R.first_block = (int)blocks;
    R.inv_n = (float)(1.0 / ((double)B * (N / 2 + 1) * R.n_frames));
    blocks += (long)B * R.n_frames;
    MV_CHECK_ARG(blocks <= 0x7fffffffL);
    if (N > max_fft) max_fft = N;
  }
  for (int r = n_res; r < STFT_MAX_RES; ++r) plan.res[r] = StftRes{0, 0, 0, 0, 0x7fffffff, 0.f};
  const size_t lds = 12 * (size_t)max_fft + 128;
  const hipStream_t s = (hipStream_t)stream;
  MV_HIP(mvi_zero_async(sums, sizeof(float) * 3 * (size_t)n_res, s));
  MV_DISPATCH(dtype, hipLaunchKernelGGL((stft_loss_kernel<T, false>), dim3((unsigned)blocks), dim3(256), lds, s, (const T*)fake,
                                        (const T*)real, sums, (float*)nullptr, plan));
  MV_LAUNCH_CHECK();
  hipLaunchKernelGGL(stft_loss_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)sums, loss, plan);
  MV_LAUNCH_CHECK();
  if (backward) {
    MV_DISPATCH(dtype, hipLaunchKernelGGL((stft_loss_kernel<T, true>), dim3((unsigned)blocks), dim3(256), lds, s, (const T*)fake,
                                          (const T*)real, sums, gwave, plan));
    MV_LAUNCH_CHECK();
  }
  return MV_OK;
}
