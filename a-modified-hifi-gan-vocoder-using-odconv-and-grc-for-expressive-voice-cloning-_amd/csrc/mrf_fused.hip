// Fused MultiReceptiveFieldBlock (the generator's "ResBlock") for the 64-channel residual stream.
//   reference arithmetic: hifigan_modified/grc_lora.py:32-68 (3x GRC_LoRA_Block 64->20, dilations d0,d1,d2)
//                         + grc_lora.py:157-163 (cat, Conv1d(60,64,1), GroupNorm(8,64), Dropout, +x)
//
// Layout: channels-last ("NTC"), x[b][t][64].  Every contraction runs on MFMA 16x16x32 with output channels on
// D rows and time on D columns (mfma.h).  Per branch, conv_g + LoRA + output_projection are folded (in fp32, at
// pack time) into one dense 3-tap dilated conv W_eff; the three branches are stacked on the 60(+4 pad) concat
// rows, so v = W_eff * x is 4 M-tiles over at most 7 distinct taps.  The residual 1x1 (64->60) and the fusion 1x1
// (60->64) follow; the fusion consumes the accumulators of the previous stage directly as its B operand (the
// k index of an MFMA may be permuted freely as long as A is packed with the same permutation).
//
// GroupNorm needs statistics over all T, twice (GN(5,20) per branch on v, GN(8,64) on the fusion output), so the
// block is three passes that each READ x ONCE and recompute:  pass 1 -> partial sums of v;  pass 2 -> partial
// sums of f;  pass 3 -> out = GN8(f) (+dropout) + x.  Nothing but x, out and a few KB of partial sums touches HBM:
// 3 reads + 1 write of the stream = 4 x 33.5 MB per block at C2 (algorithmic minimum 2 x 33.5 MB).
// Partial sums are written per workgroup and summed in a fixed order by the consumer: deterministic, no atomics.
//
// CHAIN (mv_mrf_chain_fwd_cl, the generator's three blocks in a row).  The per-block form recomputes stages 1-3 in its third
// pass only to apply GN8, an affine per (sample, channel).  The chain defers that affine to the NEXT block's first pass:
//   pass B (PASS 5) of block i:   x_i -> stages 1-3 ONCE -> writes f_i (pre-GroupNorm fusion output) + partial sums of f_i
//   pass A (PASS 4) of block i+1: x_{i+1} = a_i * f_i + b_i + x_i formed while the tile is committed to LDS (a_i, b_i from the GN8
//                                 statistics and affine of block i), written out once, stage 1 on it -> partial sums of v_{i+1}
//   pass F (PASS 6) after the last block materialises its output the same way.
// Per block: 320 MFMAs per 64-step tile instead of 512, one SiLU pass instead of two, two launches instead of three; 5 stream
// transfers (A: read f, read x, write x'; B: read x', write f) instead of 4.  Block 0's pass A is the plain statistics pass (PASS 1).
//
// Workgroup = NWAVES waves, each wave owns NTW*16 consecutive time steps of one sample and stages its own
// x tile (+halo) into a private LDS region (no block barrier on the data path); packed weights (48 KB) are
// staged once per workgroup.
#include "mrf_common.h"
#include <cstring>
#include <type_traits>
#include <cstdio>

namespace mv {

// ------------------------------------------------------------------------------------------------ pack
struct MrfRawParams {   // mirrors mv_mrf_params (include/mi355x_vocoder.h)
  const void* conv_w[3]; const void* conv_b[3]; const void* lora_A[3]; const void* lora_B[3];
  const void* lora_scaling[3]; const void* proj_w[3]; const void* proj_b[3];
  const void* norm_w[3]; const void* norm_b[3]; const void* res_w[3]; const void* res_b[3];
  const void* fusion_w; const void* fusion_b; const void* norm2_w; const void* norm2_b;
};

// folded weight of concat row `cc` (branch br, local o), input channel c, branch-local tap jj in {0,1,2}
template <typename P>
__device__ float mrf_weff(const MrfRawParams& p, int br, int o, int c, int jj, int rank) {
  const P* cw = (const P*)p.conv_w[br];   // [20][16][3]
  const P* A = (const P*)p.lora_A[br];    // [64][rank]
  const P* Bm = (const P*)p.lora_B[br];   // [rank][20]
  const P* pw = (const P*)p.proj_w[br];   // [20][20]
  const float s = ld<P>((const P*)p.lora_scaling[br]);
  float acc = 0.f;
  const int gc = c / 16;                  // groups = 4 over 64 input channels
  for (int op = 0; op < MRF_CPD; ++op) {
    float comb = 0.f;
    if (op / 5 == gc) comb = ld<P>(cw + (op * 16 + (c - gc * 16)) * 3 + jj);
    if (jj == 1) {
      float l = 0.f;
      for (int r = 0; r < rank; ++r) l += ld<P>(A + c * rank + r) * ld<P>(Bm + r * MRF_CPD + op);
      comb += s * l;
    }
    acc += ld<P>(pw + o * MRF_CPD + op) * comb;
  }
  return acc;
}

// b_eff = Wp bc + bp of concat row cc (branch br, local o): the bias of v in front of the branch GroupNorm
template <typename P>
__device__ float mrf_beff(const MrfRawParams& p, int br, int o) {
  float v = ld<P>((const P*)p.proj_b[br] + o);
  for (int op = 0; op < MRF_CPD; ++op)
    v += ld<P>((const P*)p.proj_w[br] + o * MRF_CPD + op) * ld<P>((const P*)p.conv_b[br] + op);
  return v;
}

// The bias tables b_conv and b_fus hold the biases MINUS their GroupNorm group's mean (4-channel groups of v, 8-channel groups of f).
// A GroupNorm is invariant to a constant added to a whole group, so every kernel below computes the same block - but its accumulators
// then hold v - p and f - p, p = the mean bias of the group, and the single-pass statistics (sum, sum of squares per workgroup,
// var = E[x^2] - mu^2 in fp32) are taken about that pivot at no cost in the kernels.  Unshifted, they cancel once a group's mean is a
// few tens of its stds (error of rstd 1e-5 at mean/std = 30, 5e-4 at 100), and what moves a group's mean in a trained block is the
// bias in front of the norm.  f is stored shifted too (only its GroupNorm reads it), which also keeps its f16 / hl8 rows small.
template <typename T, typename P>
__global__ __launch_bounds__(256) void mrf_pack_kernel(MrfRawParams p, MrfMeta meta, char* __restrict__ out, int rank) {
  constexpr int FS = Mma<T>::NSETS * FRAG_BYTES;
  const int nfr = MRF_CONV_FRAGS + MRF_RES_FRAGS + MRF_FUS_FRAGS;
  const int total = nfr * 512;  // 64 lanes x 8 elements per fragment
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total + MRF_TAB_FLOATS; idx += gridDim.x * blockDim.x) {
    if (idx >= total) {  // float tables
      const int ti = idx - total, which = ti / 64, cc = ti % 64;
      float v = 0.f;
      if (which == 2) {
        const P* fb = (const P*)p.fusion_b + (cc & ~7);
        float q[8];
        for (int i = 0; i < 8; ++i) q[i] = ld<P>(fb + i);
        v = q[cc & 7] - 0.125f * (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7])));
      }
      else if (which == 5) v = ld<P>((const P*)p.norm2_w + cc);
      else if (which == 6) v = ld<P>((const P*)p.norm2_b + cc);
      else if (cc < MRF_NBR * MRF_CPD) {
        const int br = cc / MRF_CPD, o = cc % MRF_CPD;
        if (which == 0) {  // b_eff minus the mean b_eff of its group (4 consecutive rows: 20 channels per branch = 5 groups)
          float q[4];
          for (int i = 0; i < 4; ++i) q[i] = mrf_beff<P>(p, br, (o & ~3) + i);
          v = q[o & 3] - 0.25f * ((q[0] + q[1]) + (q[2] + q[3]));
        } else if (which == 1) v = ld<P>((const P*)p.res_b[br] + o);
        else if (which == 3) v = ld<P>((const P*)p.norm_w[br] + o);
        else if (which == 4) v = ld<P>((const P*)p.norm_b[br] + o);
      }
      reinterpret_cast<float*>(out + (size_t)nfr * FS)[ti] = v;
      continue;
    }
    const int f = idx / 512, lane = (idx % 512) / 8, j = idx % 8;
    const int row16 = lane & 15, g = lane >> 4;
    float v = 0.f;
    if (f < MRF_CONV_FRAGS) {
      const int pair = f >> 1, ks = f & 1;
      int mt = -1, tap = -1;
      for (int a = 0; a < 4; ++a) for (int t = 0; t < meta.ntaps; ++t) if (meta.frag_of[a][t] == pair) { mt = a; tap = t; }
      if (mt >= 0) {
        const int cc = 16 * mt + row16, c = 32 * ks + 8 * g + j;
        if (cc < MRF_NBR * MRF_CPD) {
          const int br = cc / MRF_CPD, o = cc % MRF_CPD, off = meta.tap_off[tap], d = meta.dil[br];
          const int jj = (off == -d) ? 0 : (off == 0 ? 1 : (off == d ? 2 : -1));
          if (jj >= 0) v = mrf_weff<P>(p, br, o, c, jj, rank);
        }
      }
    } else if (f < MRF_CONV_FRAGS + MRF_RES_FRAGS) {
      const int ff = f - MRF_CONV_FRAGS, mt = ff >> 1, ks = ff & 1;
      const int cc = 16 * mt + row16, c = 32 * ks + 8 * g + j;
      if (cc < MRF_NBR * MRF_CPD) v = ld<P>((const P*)p.res_w[cc / MRF_CPD] + (cc % MRF_CPD) * MRF_C + c);
    } else {
      const int ff = f - MRF_CONV_FRAGS - MRF_RES_FRAGS, mo = ff >> 1, s = ff & 1;
      const int co = 16 * mo + row16;
      const int cc = 16 * (2 * s + (j >> 2)) + 4 * g + (j & 3);   // accumulator-order k permutation
      if (cc < MRF_NBR * MRF_CPD) v = ld<P>((const P*)p.fusion_w + co * (MRF_NBR * MRF_CPD) + cc);
    }
    PackW<T>::put(out + (size_t)f * FS, FRAG_BYTES, lane, j, v);
  }
}

// ------------------------------------------------------------------------------------------------ forward passes
// The reference's (and the default generator's) dilations are (1, 3, 5): for that case the tap table is a compile-time
// constant, so stage 1 becomes straight-line code that the kernel software-pipelines (operands of k-step s+1 are read
// from LDS while the MFMAs of k-step s run).  Any other dilation set takes the table from MrfMeta at run time.
constexpr int MRF_HMAX = 8;   // largest dilation the fused kernel accepts (prefetch registers are sized for it)

// one 16-byte chunk of storage elements <-> floats (8 for 16-bit storage, 4 for fp32)
template <typename T> struct Chunk;
template <> struct Chunk<bf16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const u32x4& u, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf16_lo(u[i]); f[2 * i + 1] = bf16_hi(u[i]); }
  }
  static __device__ __forceinline__ u32x4 pack(const float* f) {
    return u32x4{pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7])};
  }
};
template <> struct Chunk<f16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const u32x4& u, float* f) {
    const f16x8_t h = __builtin_bit_cast(f16x8_t, u);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
  }
  static __device__ __forceinline__ u32x4 pack(const float* f) {
    return u32x4{pack_f16(f[0], f[1]), pack_f16(f[2], f[3]), pack_f16(f[4], f[5]), pack_f16(f[6], f[7])};
  }
};
template <> struct Chunk<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const u32x4& u, float* f) {
    const f32x4 v = __builtin_bit_cast(f32x4, u);
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
  }
  static __device__ __forceinline__ u32x4 pack(const float* f) { return __builtin_bit_cast(u32x4, f32x4{f[0], f[1], f[2], f[3]}); }
};

template <typename T, int NWAVES, int NTW, int PASS, bool STD>
__global__ __launch_bounds__(NWAVES * 64) void mrf_kernel(const StT<T>* __restrict__ x, StT<T>* __restrict__ out,
                                                          const char* __restrict__ packed, MrfMeta meta,
                                                          const float* __restrict__ part5, float* __restrict__ part5_out,
                                                          const float* __restrict__ part8, float* __restrict__ part8_out,
                                                          const uint8_t* __restrict__ mask, float mask_scale,
                                                          int Tn, int nwg, int nit, float eps,
                                                          const StT<T>* __restrict__ fprev, const char* __restrict__ packed_prev) {
  using M = Mma<T>;
  using ST = StT<T>;                                  // storage type (T is the operand mode: bf16, f16, float = bf16x3, f32w16)
  using VA = typename M::VA;
  using VB = typename M::VB;
  // PASS 1/2/3: the per-block passes (statistics of v, statistics of f, output).  Chain passes: 4 = A (tile rows are
  // a*fprev + b + x, written to `out`; statistics of v), 5 = B (writes f to `out`; statistics of f), 6 = F (rows as in A, write only)
  constexpr bool RECON = (PASS == 4 || PASS == 6);
  constexpr bool NEED5 = (PASS == 2 || PASS == 3 || PASS == 5);
  constexpr bool NEED8 = (PASS == 3 || RECON);
  constexpr bool STATS_V = (PASS == 1 || PASS == 4);
  constexpr bool STATS_F = (PASS == 2 || PASS == 5);
  constexpr bool NEED_W = (PASS != 6);
  constexpr int ES = M::ES;                           // storage element size in HBM
  constexpr int FS = M::NSETS * FRAG_BYTES;
  // LDS tile rows hold MFMA operands: 16-bit storage as stored; fp32 storage PRE-SPLIT into a hi and a lo bf16 plane per row
  // (one split per element when the tile is committed, instead of one per operand read: 7 taps x 2 k-steps per column tile)
  constexpr bool SPLIT = (ES == 4);
  constexpr int LES = 2;                              // operand element size in LDS
  constexpr int PLANE = MRF_C * LES;                  // byte offset of the lo plane inside a row (SPLIT)
  constexpr int RS = (SPLIT ? 2 * PLANE : MRF_C * ES) + 32;   // padded LDS row stride: conflict-free ds_read_b128 operand reads
  constexpr int WBYTES = (MRF_CONV_FRAGS + MRF_RES_FRAGS + MRF_FUS_FRAGS) * FS;
  // fp32 statistics-of-v passes (1, 4) use the branch-conv fragments only: staging just those (64 of the 96 KB) leaves room for
  // a 256-step shared tile, i.e. NTW = 2 - every weight fragment read from LDS then feeds two column tiles (LDS reads per MFMA
  // 0.83 -> 0.5; the passes are bound by the LDS pipe: 150 operand reads for 144 MFMAs per wave and 16-step tile)
  constexpr bool CONV_ONLY = (ES == 4) && STATS_V;
  constexpr int WLB = CONV_ONLY ? MRF_CONV_FRAGS * FS : WBYTES;       // bytes of weights resident in LDS
  constexpr int TW = NTW * 16;                        // time steps per wave and iteration
  constexpr int CH = MRF_C * ES / 16;                 // 16-byte chunks per row
  // 16-bit storage: every wave stages a PRIVATE tile (TW + 2 halo rows; no workgroup barrier on the data path).  fp32 storage
  // (split operands: 2x the LDS bytes per row, 16-step tiles) shares ONE tile of NWAVES*TW + 2 halo rows per workgroup instead:
  // with private tiles 26 rows were loaded, combined and split per 16 output steps (62 % halo overhead, every wave redoing its
  // neighbours' rows); shared it is 138 rows per 128 steps, staged cooperatively between two workgroup barriers per tile, and
  // the outputs leave straight from the accumulators (no staging in rows that neighbours still read as halo).
  constexpr bool SHARED = SPLIT;
  constexpr int NT = NWAVES * 64;
  constexpr int NLD = SHARED ? ((NWAVES * TW + 2 * MRF_HMAX) * CH + NT - 1) / NT
                             : ((TW + 2 * MRF_HMAX) * CH + 63) / 64;   // prefetch registers (u32x4) per lane

  extern __shared__ __align__(16) char lds[];
  char* wl = lds;                                           // packed weights
  float* tab = reinterpret_cast<float*>(lds + WLB);         // 7 x 64 floats
  float* st5 = tab + MRF_TAB_FLOATS;                        // [16][2] mean, rstd
  float* st8 = st5 + 32;                                    // [8][2]
  float* red = st8 + 16;                                    // [NWAVES][16][2] partial sums
  char* xl = reinterpret_cast<char*>(red + NWAVES * 32);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, wg = blockIdx.x;
  const int H = meta.halo;
  const int rows = (SHARED ? NWAVES * TW : TW) + 2 * H;                  // rows of one staged tile
  char* xw = xl + (size_t)wid * (SHARED ? TW : rows) * RS;              // row 0 of this wave's window (its first halo row)
  char* xs = SHARED ? xl : xw;                                           // base of the tile this thread helps to stage
  const int sidx = SHARED ? tid : lane;                                  // staging piece index of this thread: sidx + SSTEP * i
  constexpr int SSTEP = SHARED ? NT : 64;
  const int own_rows = SHARED ? NWAVES * TW : TW;
  const ST* xb = x + (size_t)b * Tn * MRF_C;

  // ---- software pipeline: the NEXT tile's rows travel HBM -> registers while the current tile is computed
  using CK = Chunk<ST>;
  constexpr int NPF = RECON ? NLD : 1;
  u32x4 pre[NLD], pref[NPF];                         // x rows; chain passes A / F: the previous block's f rows as well
  const ST* fb = RECON ? fprev + (size_t)b * Tn * MRF_C : nullptr;
  ST* ob = out + (size_t)b * Tn * MRF_C;
  float ra[CK::N], rb[CK::N];                        // chain passes A / F: this lane's chunk of the deferred GN8 affine (set below)
  auto tile_t0 = [&](int it) { return ((wg * nit + it) * NWAVES + wid) * TW; };     // first output step of this WAVE
  auto stage_t0 = [&](int it) { return SHARED ? (wg * nit + it) * NWAVES * TW : tile_t0(it); };   // ... of the staged tile
  auto issue = [&](int it) {
    const int t0 = stage_t0(it);
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = sidx + SSTEP * i;
      const int r = idx / CH, ch = idx % CH;
      const int t = t0 - H + r;
      u32x4 v = {0u, 0u, 0u, 0u}, vf = {0u, 0u, 0u, 0u};
      if (idx < rows * CH && t >= 0 && t < Tn) {
        v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(xb + (size_t)t * MRF_C) + ch * 16);
        if constexpr (RECON) vf = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(fb + (size_t)t * MRF_C) + ch * 16);
      }
      pre[i] = v;
      if constexpr (RECON) pref[i] = vf;
    }
  };
  auto commit = [&](int t0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = sidx + SSTEP * i;
      const int r = idx / CH, ch = idx % CH;           // ch == lane % CH for every i (SSTEP % CH == 0): ra / rb are per lane
      if (idx < rows * CH) {
        u32x4 val = pre[i];
        if constexpr (RECON) {
          // x' = a * f + b + x: the previous block's GroupNorm(8,64) + residual (grc_lora.py:161-163), applied on the way in
          const int t = t0 - H + r;
          float fx[CK::N], ff[CK::N];
          CK::unpack(pre[i], fx);
          CK::unpack(pref[i], ff);
          const bool inside = t >= 0 && t < Tn;         // rows outside the sample are the conv's zero padding, not b
#pragma unroll
          for (int j = 0; j < CK::N; ++j) fx[j] = inside ? ra[j] * ff[j] + rb[j] + fx[j] : 0.f;
          val = CK::pack(fx);
          if (r >= H && r < H + own_rows && inside)      // the tile's own (non-halo) rows leave for HBM here, once
            *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(ob + (size_t)t * MRF_C) + ch * 16) = val;
        }
        if constexpr (PASS != 6) {
          if constexpr (SPLIT) {
            u32x2 hi, lo;
            M::split4(__builtin_bit_cast(f32x4, val), hi, lo);
            *reinterpret_cast<u32x2*>(xs + r * RS + ch * 8) = hi;
            *reinterpret_cast<u32x2*>(xs + r * RS + PLANE + ch * 8) = lo;
          } else {
            *reinterpret_cast<u32x4*>(xs + r * RS + ch * 16) = val;
          }
        }
      }
    }
  };
  issue(0);

  // ---- stage packed weights + tables (whole workgroup, once): all global loads of a thread in flight together
  {
    constexpr int N16 = (WLB + MRF_TAB_FLOATS * 4) / 16;      // resident fragments, then the tables (behind ALL fragments in `packed`)
    constexpr int PER = (N16 + NWAVES * 64 - 1) / (NWAVES * 64);
    const u32x4* src = reinterpret_cast<const u32x4*>(packed);
    u32x4* dst = reinterpret_cast<u32x4*>(lds);
    u32x4 wv[PER];
    if constexpr (NEED_W) {
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        int idx = tid + i * NWAVES * 64;
        idx = idx < N16 ? idx : N16 - 1;
        wv[i] = src[idx < WLB / 16 ? idx : idx + (WBYTES - WLB) / 16];
      }
    }
    // GroupNorm statistics from the previous passes' partial sums: one partial per thread, then a fixed-order sum in LDS
    float2 pp = {0.f, 0.f};
    const int pi = tid >> 4, pq = tid & 15;                 // (workgroup index, group) for GN5; GN8 uses threads 256..
    if (NEED5 && pi < nwg && tid < 256) pp = *reinterpret_cast<const float2*>(part5 + ((size_t)(b * nwg + pi) * 16 + pq) * 2);
    float2 pp8 = {0.f, 0.f};
    const int t8 = (NWAVES * 64 >= 512) ? tid - 256 : tid, pi8 = t8 >> 3, pq8 = t8 & 7;   // (4-wave workgroups: the GN5 threads load these too)
    if (NEED8 && t8 >= 0 && pi8 < nwg && t8 < 128) pp8 = *reinterpret_cast<const float2*>(part8 + ((size_t)(b * nwg + pi8) * 8 + pq8) * 2);
    if constexpr (NEED_W) {
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int idx = tid + i * NWAVES * 64;
        if (idx < N16) dst[idx] = wv[i];
      }
    }
    // xl (the waves' x tiles) is not written before the first commit(): use its head as scratch for the partials
    float2* sc5 = reinterpret_cast<float2*>(xl);
    float2* sc8 = sc5 + 256;
    if (NEED5 && tid < 256) sc5[tid] = pp;
    if (NEED8 && t8 >= 0 && t8 < 128) sc8[t8] = pp8;
  }
  const bool fast_stats = nwg <= 16 && NWAVES * 64 >= 256;
  if (NEED5 || NEED8) __syncthreads();
  if (NEED5 && tid < 16) {
    float s1 = 0.f, s2 = 0.f;
    if (fast_stats) {
      const float2* sc5 = reinterpret_cast<const float2*>(xl);
      for (int i = 0; i < nwg; ++i) { s1 += sc5[i * 16 + tid].x; s2 += sc5[i * 16 + tid].y; }
    } else {
      for (int i = 0; i < nwg; ++i) {
        s1 += part5[((size_t)(b * nwg + i) * 16 + tid) * 2];
        s2 += part5[((size_t)(b * nwg + i) * 16 + tid) * 2 + 1];
      }
    }
    const float n = 4.f * (float)Tn, mu = s1 / n;
    const float var = fmaxf(s2 / n - mu * mu, 0.f);
    st5[tid * 2] = mu;
    st5[tid * 2 + 1] = rsqrtf(var + eps);
  }
  if (NEED8 && tid >= 64 && tid < 72) {
    const int q = tid - 64;
    float s1 = 0.f, s2 = 0.f;
    if (fast_stats) {
      const float2* sc8 = reinterpret_cast<const float2*>(xl) + 256;
      for (int i = 0; i < nwg; ++i) { s1 += sc8[i * 8 + q].x; s2 += sc8[i * 8 + q].y; }
    } else {
      for (int i = 0; i < nwg; ++i) {
        s1 += part8[((size_t)(b * nwg + i) * 8 + q) * 2];
        s2 += part8[((size_t)(b * nwg + i) * 8 + q) * 2 + 1];
      }
    }
    const float n = 8.f * (float)Tn, mu = s1 / n;
    const float var = fmaxf(s2 / n - mu * mu, 0.f);
    st8[q * 2] = mu;
    st8[q * 2 + 1] = rsqrtf(var + eps);
  }
  __syncthreads();

  const float* b_conv = tab, *b_res = tab + 64, *b_fus = tab + 128;
  const float* g5 = tab + 192, *be5 = tab + 256, *g8 = tab + 320, *be8 = tab + 384;
  const char* xcol = xw + (size_t)(col + H) * RS + 8 * g * LES;  // this lane's B-operand base
  if constexpr (RECON) {
    // deferred GroupNorm(8,64) of the PREVIOUS block for this lane's chunk of channels: a = rstd * gamma, b = beta - mean * a
    const float* tprev = reinterpret_cast<const float*>(packed_prev + WBYTES);
    const int c0 = (lane % CH) * CK::N;
#pragma unroll
    for (int j = 0; j < CK::N; ++j) {
      const int c = c0 + j, q = c >> 3;
      ra[j] = st8[q * 2 + 1] * tprev[320 + c];
      rb[j] = tprev[384 + c] - st8[q * 2] * ra[j];
    }
  }

  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};   // statistics partials (passes 1, 2)

  for (int it = 0; it < nit; ++it) {
    const int t0 = tile_t0(it);
    if constexpr (SHARED && PASS != 6) { if (it > 0) __syncthreads(); }   // every wave is done reading the previous shared tile
    commit(stage_t0(it));           // this tile: registers -> LDS (chain A / F: + x' -> HBM)
    if (it + 1 < nit) issue(it + 1);
    if constexpr (PASS == 6) continue;
    if constexpr (SHARED) __syncthreads(); else __builtin_amdgcn_wave_barrier();

    // ---- stage 1: v[cc][t] = b_eff + sum_{tap,c} W_eff[cc][tap][c] x[t+off(tap)][c]
    f32x4 v[4][NTW];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const f32x4 bi = *reinterpret_cast<const f32x4*>(b_conv + 16 * m + 4 * g);
#pragma unroll
      for (int n = 0; n < NTW; ++n) v[m][n] = bi;
    }
    if (STD) {
      // straight-line, software-pipelined: step s = (tap, ks); two operand sets alternate
      VB bfr[2][NTW];
      VA afr[2][4];
      auto ld_step = [&](int sidx, int set) {
        const int tap = sidx >> 1, ks = sidx & 1;
#pragma unroll
        for (int n = 0; n < NTW; ++n) bfr[set][n] = M::load_bp(xcol + (n * 16 + mrf_std_off(tap)) * RS + ks * 32 * LES, PLANE);
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (mrf_std_frag(m, tap) >= 0) afr[set][m] = M::load_a(wl + (size_t)(mrf_std_frag(m, tap) * 2 + ks) * FS + lane * 16, FRAG_BYTES);
      };
      ld_step(0, 0);
#pragma unroll
      for (int sidx = 0; sidx < 14; ++sidx) {
        if (sidx + 1 < 14) ld_step(sidx + 1, (sidx + 1) & 1);
        // keep the NEXT step's operand reads above this step's MFMAs: left alone, the scheduler sinks every ds_read to just in
        // front of its first use (r, s_waitcnt lgkmcnt(0), MFMA, r, wait, MFMA ... in the ISA) and each MFMA pays an LDS round trip
        __builtin_amdgcn_sched_barrier(0);
        const int tap = sidx >> 1, set = sidx & 1;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (mrf_std_frag(m, tap) >= 0) {
#pragma unroll
            for (int n = 0; n < NTW; ++n) v[m][n] = M::mma(afr[set][m], bfr[set][n], v[m][n]);
          }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else
    for (int tap = 0; tap < meta.ntaps; ++tap) {
      const int off = meta.tap_off[tap];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // every operand of this k-step first (independent LDS reads in flight together), then the MFMAs
        VB bf[NTW];
        VA af[4];
#pragma unroll
        for (int n = 0; n < NTW; ++n) bf[n] = M::load_bp(xcol + (n * 16 + off) * RS + ks * 32 * LES, PLANE);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int fo = meta.frag_of[m][tap];
          af[m] = M::load_a(wl + (size_t)((fo >= 0 ? fo : 0) * 2 + ks) * FS + lane * 16, FRAG_BYTES);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (meta.frag_of[m][tap] >= 0) {
#pragma unroll
            for (int n = 0; n < NTW; ++n) v[m][n] = M::mma(af[m], bf[n], v[m][n]);
          }
        }
      }
    }

    if (STATS_V) {
      // partial sums of v per GN(5,20) group: concat rows 16m+4g..+3 are exactly group 4m+g
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          const bool ok = (t0 + n * 16 + col) < Tn;
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float q = ok ? v[m][n][r] : 0.f; s1[m] += q; s2[m] += q * q; }
        }
      continue;
    }

    // ---- stage 2: c = SiLU(GN5(v)) + b_res + W_res x : activate in place, then let the residual 1x1 accumulate
    //      straight onto the activated values (no second accumulator set)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float mu = st5[(4 * m + g) * 2], rs = st5[(4 * m + g) * 2 + 1];
      const f32x4 ga = *reinterpret_cast<const f32x4*>(g5 + 16 * m + 4 * g);
      const f32x4 be = *reinterpret_cast<const f32x4*>(be5 + 16 * m + 4 * g);
      const f32x4 br = *reinterpret_cast<const f32x4*>(b_res + 16 * m + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = rs * ga[r], sh = be[r] - mu * sc;
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          const float w = v[m][n][r] * sc + sh;
          v[m][n][r] = w * __builtin_amdgcn_rcpf(1.f + __expf(-w)) + br[r];   // SiLU (v_exp + v_rcp, 1 ulp)
        }
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      VB bf[NTW];
      VA af[4];
#pragma unroll
      for (int n = 0; n < NTW; ++n) bf[n] = M::load_bp(xcol + (n * 16) * RS + ks * 32 * LES, PLANE);
#pragma unroll
      for (int m = 0; m < 4; ++m) af[m] = M::load_a(wl + (size_t)(MRF_CONV_FRAGS + m * 2 + ks) * FS + lane * 16, FRAG_BYTES);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NTW; ++n) v[m][n] = M::mma(af[m], bf[n], v[m][n]);
    }

    // ---- stage 3: f[co][t] = b_fus + sum_cc W_fus[co][cc] c[cc][t]   (c fed straight from the accumulators)
    f32x4 f[4][NTW];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const f32x4 bi = *reinterpret_cast<const f32x4*>(b_fus + 16 * m + 4 * g);
#pragma unroll
      for (int n = 0; n < NTW; ++n) f[m][n] = bi;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      VB cb[NTW];
#pragma unroll
      for (int n = 0; n < NTW; ++n) cb[n] = M::from_acc(v[2 * s][n], v[2 * s + 1][n]);
      VA af[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) af[m] = M::load_a(wl + (size_t)(MRF_CONV_FRAGS + MRF_RES_FRAGS + m * 2 + s) * FS + lane * 16, FRAG_BYTES);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NTW; ++n) f[m][n] = M::mma(af[m], cb[n], f[m][n]);
    }

    if (STATS_F) {
      // partial sums of f per GN(8,64) group: rows 16m+4g+r -> group 2m + (g>>1)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          const bool ok = (t0 + n * 16 + col) < Tn;
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float q = ok ? f[m][n][r] : 0.f; s1[m] += q; s2[m] += q * q; }
        }
      if constexpr (PASS == 2) continue;
    }

    if constexpr (PASS == 5) {
      // chain pass B: f itself leaves for HBM (its GroupNorm is applied by the next block's pass A); staged in this wave's tile rows
      // (the x tile is dead: its last reader was the residual 1x1 above) and streamed out as whole rows like the output below
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          const float o[4] = {f[m][n][0], f[m][n][1], f[m][n][2], f[m][n][3]};
          if constexpr (SHARED) {     // straight from the accumulators: 4 channels x fp32 = 16 B per lane, 64 B runs per row
            const int t = t0 + n * 16 + col;
            if (t < Tn) M::store4(ob + (size_t)t * MRF_C + 16 * m + 4 * g, o);
          } else {
            M::store4(xw + (size_t)(n * 16 + col + H) * RS + (16 * m + 4 * g) * ES, o);
          }
        }
    }

    // ---- stage 4 (pass 3): out = GN8(f) * keep/(1-p) + x, written IN PLACE over this wave's x tile, then streamed
    //      to HBM as whole 128/256-byte rows (16 B per lane, 1 KB per wave instruction)
    // the dropout-mask test is hoisted out of the 64-element loop (inference passes no mask)
    auto stage4 = [&](auto mask_c) {
      constexpr bool HAS_MASK = decltype(mask_c)::value;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int q = 2 * m + (g >> 1);
        const float mu = st8[q * 2], rs = st8[q * 2 + 1];
        const f32x4 ga = *reinterpret_cast<const f32x4*>(g8 + 16 * m + 4 * g);
        const f32x4 be = *reinterpret_cast<const f32x4*>(be8 + 16 * m + 4 * g);
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          const int t = t0 + n * 16 + col;
          char* rowp = xw + (size_t)(n * 16 + col + H) * RS;
          float xr[4], o[4];
          if constexpr (SPLIT) {
            float lo4[4];
            M::load4p(rowp + (16 * m + 4 * g) * LES, xr);
            M::load4p(rowp + PLANE + (16 * m + 4 * g) * LES, lo4);
#pragma unroll
            for (int r = 0; r < 4; ++r) xr[r] += lo4[r];
          } else {
            M::load4(rowp + (16 * m + 4 * g) * ES, xr);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // explicit fmas: left to the compiler's contraction, the masked and the maskless instantiation of this lambda fused
            // different elements (fp32: v_mul + v_pk_add for half of them without a mask, v_fmac for all with one), so a mask of
            // ones did not reproduce the maskless call bit for bit (tests/test_gpu_mrf_arms.py)
            const float sc = rs * ga[r];
            float w = __builtin_fmaf(f[m][n][r], sc, __builtin_fmaf(-mu, sc, be[r]));
            if (HAS_MASK) w = (t < Tn && mask[((size_t)b * Tn + t) * MRF_C + 16 * m + 4 * g + r]) ? w * mask_scale : 0.f;
            o[r] = w + xr[r];
          }
          if constexpr (SPLIT) {
            // the fp32 output row overlaps the hi/lo planes of OTHER channels of the same row: keep the results in registers
            // until every residual read of the tile has been issued (second loop below)
#pragma unroll
            for (int r = 0; r < 4; ++r) f[m][n][r] = o[r];
          } else {
            M::store4(rowp + (16 * m + 4 * g) * ES, o);    // same bytes this lane has just read
          }
        }
      }
      if constexpr (SPLIT) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < NTW; ++n) {
            const float o[4] = {f[m][n][0], f[m][n][1], f[m][n][2], f[m][n][3]};
            const int t = t0 + n * 16 + col;
            if (t < Tn) M::store4(ob + (size_t)t * MRF_C + 16 * m + 4 * g, o);     // shared tile: straight to HBM
          }
      }
    };
    if constexpr (PASS == 3) { if (mask) stage4(std::true_type{}); else stage4(std::false_type{}); }
    if constexpr (!SHARED) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < (TW * CH) / 64; ++i) {
        const int idx = lane + 64 * i;
        const int r = idx / CH, ch = idx % CH;
        const int t = t0 + r;
        const u32x4 val = *reinterpret_cast<const u32x4*>(xw + (size_t)(r + H) * RS + ch * 16);
        if (t < Tn) *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(ob + (size_t)t * MRF_C) + ch * 16) = val;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }

  if (STATS_V) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) { s1[m] += __shfl_xor(s1[m], o, 64); s2[m] += __shfl_xor(s2[m], o, 64); }
    }
    if (col == 0) {
#pragma unroll
      for (int m = 0; m < 4; ++m) { red[(wid * 16 + 4 * m + g) * 2] = s1[m]; red[(wid * 16 + 4 * m + g) * 2 + 1] = s2[m]; }
    }
    __syncthreads();
    if (tid < 32) {
      float a = 0.f;
      for (int w = 0; w < NWAVES; ++w) a += red[w * 32 + tid];
      part5_out[(size_t)(b * nwg + wg) * 32 + tid] = a;
    }
  }
  if (STATS_F) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int o = 1; o <= 16; o <<= 1) { s1[m] += __shfl_xor(s1[m], o, 64); s2[m] += __shfl_xor(s2[m], o, 64); }
    }
    if (col == 0 && (g & 1) == 0) {
#pragma unroll
      for (int m = 0; m < 4; ++m) { red[(wid * 8 + 2 * m + (g >> 1)) * 2] = s1[m]; red[(wid * 8 + 2 * m + (g >> 1)) * 2 + 1] = s2[m]; }
    }
    __syncthreads();
    if (tid < 16) {
      float a = 0.f;
      for (int w = 0; w < NWAVES; ++w) a += red[w * 16 + tid];
      part8_out[(size_t)(b * nwg + wg) * 16 + tid] = a;
    }
  }
}

// workgroups per sample and tiles per wave: aim at one persistent workgroup per CU when the batch allows it
static inline void mrf_geometry(int B, int Tn, int tile_t, int* nwg, int* nit) {
  const int ntiles = cdiv(Tn, tile_t);
  int it = 1;
  // up to 8 tiles per workgroup: the prologue (48-96 KB of packed weights into LDS) is paid once per workgroup, and at fp32's 128-step
  // workgroup tiles the C2 batch is 2048 tiles - 512 workgroups of 4 tiles staged the weights twice per CU and pass
  while (it < 8 && (long)B * cdiv(ntiles, it) > 256 && cdiv(ntiles, it * 2) >= 1 && ntiles >= it * 2) it *= 2;
  *nit = it;
  *nwg = cdiv(ntiles, it);
}

// The geometry of the tile form for one instantiation <T, NWAVES, NTW>, for the block entry (nblocks = 1, chain false) and the chain:
// workgroups and iterations, dynamic LDS, the chain's wide first pass, the grid.  mrf_launch and mrf_chain_launch launch what this
// returns and mv_mrf_plan reports it; MV_ERR_UNSUPPORTED where the shared tile does not fit 160 KB or a halo exceeds MRF_HMAX.
template <typename T, int NWAVES, int NTW>
static int mrf_tile_plan(const MrfMeta* metas, int nblocks, bool chain, int B, int Tn, MrfPlan* p) {
  using M = Mma<T>;
  constexpr int FS = M::NSETS * FRAG_BYTES;
  constexpr int RS = (M::ES == 4 ? 2 * MRF_C * 2 : MRF_C * M::ES) + 32;   // as in the kernel
  int nwg, nit, hmax = 0, stdm = 0;
  mrf_geometry(B, Tn, NWAVES * NTW * 16, &nwg, &nit);
  for (int i = 0; i < nblocks; ++i) {
    hmax = metas[i].halo > hmax ? metas[i].halo : hmax;
    if (mrf_meta_is_std(metas[i])) stdm |= 1 << i;
  }
  const size_t tile_rows = M::ES == 4 ? (size_t)NWAVES * NTW * 16 + 2 * hmax : (size_t)NWAVES * (NTW * 16 + 2 * hmax);
  const size_t lds = (size_t)(MRF_CONV_FRAGS + MRF_RES_FRAGS + MRF_FUS_FRAGS) * FS + MRF_TAB_FLOATS * 4 + (32 + 16) * 4 +
                     (size_t)NWAVES * 32 * 4 + tile_rows * RS;
  if (lds > 160 * 1024 || hmax > MRF_HMAX) return MV_ERR_UNSUPPORTED;
  // fp32 chain: the statistics-of-v pass of block 0 keeps only the branch-conv fragments in LDS and runs 32-step wave tiles (see the
  // kernel); same workgroup count, half the iterations, so the partial-sum buffers line up with the 16-step passes
  constexpr bool WIDE_OK = (M::ES == 4) && NTW == 1;
  const size_t lds_wide = (size_t)MRF_CONV_FRAGS * FS + MRF_TAB_FLOATS * 4 + (32 + 16) * 4 + (size_t)NWAVES * 32 * 4 +
                          ((size_t)NWAVES * 2 * 16 + 2 * hmax) * RS;
  const bool wide = chain && WIDE_OK && nit >= 2 && nit % 2 == 0 && lds_wide <= 160 * 1024 && Tn % (NWAVES * 32) == 0;
  *p = MrfPlan{};
  p->form = 0; p->nwaves = NWAVES; p->ntw = NTW; p->std_mask = stdm; p->nwg = nwg; p->nit = nit; p->wide = wide;
  p->lds = (int)lds; p->lds_wide = wide ? (int)lds_wide : 0; p->gx = nwg; p->gy = B; p->hmax = hmax;
  p->kind = -1; p->out_family = -1; p->row_form = -1;
  return MV_OK;
}

template <typename T, int NWAVES, int NTW>
static int mrf_launch(const void* x, void* out, const void* packed, const MrfMeta& meta, float* ws,
                      const uint8_t* mask, float mask_scale, int B, int Tn, float eps, hipStream_t stream, MrfPlan* plan) {
  MrfPlan g;
  const int prc = mrf_tile_plan<T, NWAVES, NTW>(&meta, 1, false, B, Tn, &g);
  if (prc != MV_OK) return prc;
  if (plan) { g.launches = 3; *plan = g; return MV_OK; }
  const int nwg = g.nwg, nit = g.nit;
  const size_t lds = (size_t)g.lds;
  float* part5 = ws;
  float* part8 = ws + (size_t)B * nwg * 32;
  dim3 grid(g.gx, g.gy), block(NWAVES * 64);
  const bool stdm = g.std_mask & 1;
  auto k1 = stdm ? mrf_kernel<T, NWAVES, NTW, 1, true> : mrf_kernel<T, NWAVES, NTW, 1, false>;
  auto k2 = stdm ? mrf_kernel<T, NWAVES, NTW, 2, true> : mrf_kernel<T, NWAVES, NTW, 2, false>;
  auto k3 = stdm ? mrf_kernel<T, NWAVES, NTW, 3, true> : mrf_kernel<T, NWAVES, NTW, 3, false>;
  static size_t lds_set[2] = {0, 0};   // per instantiation: raise the dynamic-LDS limit once (and again if a larger halo needs it)
  if (lds > lds_set[stdm]) {
    (void)hipFuncSetAttribute((const void*)k1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)k3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    lds_set[stdm] = lds;
  }
  using ST = StT<T>;
  hipLaunchKernelGGL(k1, grid, block, lds, stream, (const ST*)x, (ST*)out, (const char*)packed, meta, nullptr, part5,
                     nullptr, nullptr, nullptr, 1.f, Tn, nwg, nit, eps, (const ST*)nullptr, (const char*)nullptr);
  hipLaunchKernelGGL(k2, grid, block, lds, stream, (const ST*)x, (ST*)out, (const char*)packed, meta, part5, nullptr,
                     nullptr, part8, nullptr, 1.f, Tn, nwg, nit, eps, (const ST*)nullptr, (const char*)nullptr);
  hipLaunchKernelGGL(k3, grid, block, lds, stream, (const ST*)x, (ST*)out, (const char*)packed, meta, part5, nullptr,
                     part8, nullptr, mask, mask_scale, Tn, nwg, nit, eps, (const ST*)nullptr, (const char*)nullptr);
  return MV_OK;
}

// ---- the chained form: blocks 0..n-1 in a row, GroupNorm(8,64) of block i deferred into pass A of block i+1 (header comment)

template <typename T, int NWAVES, int NTW, int PASS>
static void mrf_chain_pass(bool stdm, dim3 grid, size_t lds, hipStream_t stream, const StT<T>* x, StT<T>* out, const char* packed,
                           const MrfMeta& meta, const float* p5, float* p5o, const float* p8, float* p8o, int Tn, int nwg, int nit,
                           float eps, const StT<T>* fprev, const char* packed_prev) {
  auto k = stdm ? mrf_kernel<T, NWAVES, NTW, PASS, true> : mrf_kernel<T, NWAVES, NTW, PASS, false>;
  static size_t lds_set[2] = {0, 0};
  if (lds > lds_set[stdm]) {
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    lds_set[stdm] = lds;
  }
  hipLaunchKernelGGL(k, grid, dim3(NWAVES * 64), lds, stream, x, out, packed, meta, p5, p5o, p8, p8o, (const uint8_t*)nullptr, 1.f, Tn,
                     nwg, nit, eps, fprev, packed_prev);
}

// deferred GroupNorm(8,64) affine of the chain's last block, for a consumer that applies it itself: ab[b][0][c] = rstd * gamma,
// ab[b][1][c] = beta - mean * rstd * gamma (fixed-order sum of the per-workgroup partials)
__global__ __launch_bounds__(64) void mrf_affine_kernel(const float* __restrict__ part8, const float* __restrict__ tab,
                                                        float* __restrict__ ab, int nwg, int Tn, float eps) {
  const int b = blockIdx.x, c = threadIdx.x, q = c >> 3;
  float s1 = 0.f, s2 = 0.f;
  for (int i = 0; i < nwg; ++i) {
    s1 += part8[((size_t)(b * nwg + i) * 8 + q) * 2];
    s2 += part8[((size_t)(b * nwg + i) * 8 + q) * 2 + 1];
  }
  const float n = 8.f * (float)Tn, mu = s1 / n;
  const float rs = rsqrtf(fmaxf(s2 / n - mu * mu, 0.f) + eps);
  const float a = rs * tab[320 + c];
  ab[(size_t)b * 128 + c] = a;
  ab[(size_t)b * 128 + 64 + c] = tab[384 + c] - mu * a;
}

// The validated request of the two chain entries, what the caller wants at the end of the chain, and the chain in its tile form.
struct MrfChainReq {
  const void* x; void* out; const void* const* packed; MrfMeta metas[8]; int nblocks; char* ws; int B, T; float eps;
  int dtype;                 // storage dtype (MV_F32_W16P decoded: MV_F32_W16 with x_pair_in)
  bool x_pair_in;            // x arrives as pair rows (streaming form only)
  hipStream_t stream;
};
enum MrfChainKind {
  MATERIALIZE,               // pass F writes the last block's output to `out`
  PASSES_ONLY,               // the passes run and leave (f, x, partial sums) in the workspace; nothing else is launched
  TAIL_WITH_AB,              // no pass F: the caller gets the tail, and mrf_affine_kernel writes the deferred affine to the workspace
  TAIL_WITH_PARTIALS         // no pass F: the caller gets the tail and forms the affine itself from the partial sums
};

template <typename T, int NWAVES, int NTW>
static int mrf_chain_launch(const MrfChainReq& r, const MrfChainWs& lay, MrfChainKind kind, MrfChainTail* tail, MrfPlan* plan) {
  const void* const* packed = r.packed;
  const MrfMeta* metas = r.metas;
  char* const ws = r.ws;
  const int nblocks = r.nblocks, B = r.B, Tn = r.T;
  const float eps = r.eps;
  const hipStream_t stream = r.stream;
  using M = Mma<T>;
  constexpr int FS = M::NSETS * FRAG_BYTES;
  MrfPlan g;
  const int prc = mrf_tile_plan<T, NWAVES, NTW>(metas, nblocks, true, B, Tn, &g);
  if (prc != MV_OK) return prc;
  const int nwg = g.nwg, nit = g.nit;
  const size_t lds = (size_t)g.lds, lds_wide = (size_t)g.lds_wide;
  const bool wide = g.wide;
  using ST = StT<T>;
  ST* fbuf = reinterpret_cast<ST*>(ws + lay.f);
  ST* xbuf[2] = {reinterpret_cast<ST*>(ws + lay.x[0]), reinterpret_cast<ST*>(ws + lay.x[1])};
  float* part5 = reinterpret_cast<float*>(ws + lay.part5);
  float* part8 = part5 + (size_t)B * nwg * 32;
  const dim3 grid(g.gx, g.gy);
  constexpr bool WIDE_OK = (M::ES == 4) && NTW == 1;   // the wide pass (mrf_tile_plan) exists for this instantiation
  if (plan) {                                        // the dry run: what the lines below would launch, and the tail they would hand on
    g.kind = kind;
    g.launches = 2 * nblocks + (kind == MATERIALIZE || kind == TAIL_WITH_AB ? 1 : 0);
    *plan = g;
    const ST* xl = nblocks > 1 ? xbuf[(nblocks - 1) & 1] : (const ST*)r.x;
    if (kind == TAIL_WITH_AB) *tail = MrfChainTail{fbuf, xl, MRF_ROWS_FP32, nullptr, nullptr, 0};
    else if (kind != MATERIALIZE) *tail = MrfChainTail{fbuf, xl, MRF_ROWS_FP32, part8, nullptr, nwg};
    return MV_OK;
  }
  const ST* xi = (const ST*)r.x;                     // x_i: the input of block i
  for (int i = 0; i < nblocks; ++i) {
    const bool stdm = (g.std_mask >> i) & 1;
    const char* pk = (const char*)packed[i];
    if (i == 0) {
      if (wide)
        mrf_chain_pass<T, NWAVES, (WIDE_OK ? 2 : NTW), 1>(stdm, grid, lds_wide, stream, xi, (ST*)nullptr, pk, metas[i], nullptr, part5, nullptr,
                                                          nullptr, Tn, nwg, nit / 2, eps, nullptr, nullptr);
      else
        mrf_chain_pass<T, NWAVES, NTW, 1>(stdm, grid, lds, stream, xi, (ST*)nullptr, pk, metas[i], nullptr, part5, nullptr, nullptr, Tn, nwg,
                                          nit, eps, nullptr, nullptr);
    } else {
      ST* xn = xbuf[i & 1];                          // pass A: x_i = GN8_{i-1}(f_{i-1}) + x_{i-1}, written once; statistics of v_i
      // (pass A at 32-step tiles needs 256 VGPRs + spills: 50 vs 43 us)
      mrf_chain_pass<T, NWAVES, NTW, 4>(stdm, grid, lds, stream, xi, xn, pk, metas[i], nullptr, part5, part8, nullptr, Tn, nwg, nit, eps,
                                        fbuf, (const char*)packed[i - 1]);
      xi = xn;
    }
    // pass B: stages 1-3 once, f_i -> fbuf, statistics of f_i
    mrf_chain_pass<T, NWAVES, NTW, 5>(stdm, grid, lds, stream, xi, fbuf, pk, metas[i], part5, nullptr, nullptr, part8, Tn, nwg, nit, eps,
                                      nullptr, nullptr);
  }
  if (kind != MATERIALIZE) {
    constexpr size_t WB = (size_t)(MRF_CONV_FRAGS + MRF_RES_FRAGS + MRF_FUS_FRAGS) * FS;
    const float* tabp = reinterpret_cast<const float*>((const char*)packed[nblocks - 1] + WB);
    if (kind == TAIL_WITH_AB) {
      hipLaunchKernelGGL(mrf_affine_kernel, dim3(B), dim3(64), 0, stream, part8, tabp, reinterpret_cast<float*>(ws + lay.ab), nwg, Tn, eps);
      *tail = MrfChainTail{fbuf, xi, MRF_ROWS_FP32, nullptr, nullptr, 0};
    } else {
      *tail = MrfChainTail{fbuf, xi, MRF_ROWS_FP32, part8, tabp, nwg};
    }
    return MV_OK;
  }
  MrfMeta mf = metas[nblocks - 1];
  mf.halo = 0;                                       // pass F touches this wave's own rows only
  mrf_chain_pass<T, NWAVES, NTW, 6>(true, grid, lds, stream, xi, (ST*)r.out, (const char*)packed[nblocks - 1], mf, nullptr, nullptr, part8,
                                    nullptr, Tn, nwg, nit, eps, fbuf, (const char*)packed[nblocks - 1]);
  return MV_OK;
}

}  // namespace mv

using namespace mv;

extern "C" size_t mv_mrf_packed_bytes(int dtype) {
  switch (dtype) {
    case MV_F32: return mrf_packed_bytes<float>();
    case MV_BF16: return mrf_packed_bytes<bf16>();
    case MV_F16: case MV_F32_W16: return mrf_packed_bytes<f16>();
    default: return 0;
  }
}

// tile geometry per storage type: bf16/f16: 8 waves x 64 steps; fp32 (split operands, 2x LDS): 8 x 16 or 4 x 32 steps
static inline int mrf_tile_t(int dtype) { return dtype == MV_F32_W16 ? 4 * 1 * 16 : dtype == MV_F32 ? 8 * 1 * 16 : 8 * 4 * 16; }
// f32w16 tile form (chains the streaming form does not take): 8 waves x 32 steps (the single-f16 weight image is 48 KB, so a
// 256-step shared tile fits)

extern "C" size_t mv_mrf_workspace_bytes(int B, int T_, int dtype) {
  const int ntiles = cdiv(T_, mrf_tile_t(dtype));   // upper bound on workgroups per sample
  return (size_t)B * ntiles * (32 + 16) * sizeof(float);
}

template <typename T>
static int mrf_pack_dispatch(const mv_mrf_params* prm, const MrfMeta& meta, void* packed, int rank, int param_dtype,
                             hipStream_t stream) {
  MrfRawParams p;
  static_assert(sizeof(MrfRawParams) == sizeof(mv_mrf_params), "mv_mrf_params layout");
  std::memcpy(&p, prm, sizeof(p));
  const dim3 grid(48), block(256);
  switch (param_dtype) {
    case MV_F32: hipLaunchKernelGGL((mrf_pack_kernel<T, float>), grid, block, 0, stream, p, meta, (char*)packed, rank); break;
    case MV_BF16: hipLaunchKernelGGL((mrf_pack_kernel<T, bf16>), grid, block, 0, stream, p, meta, (char*)packed, rank); break;
    case MV_F16: hipLaunchKernelGGL((mrf_pack_kernel<T, f16>), grid, block, 0, stream, p, meta, (char*)packed, rank); break;
    default: return MV_ERR_DTYPE;
  }
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_mrf_pack(const mv_mrf_params* params, int param_dtype, const int* dilations, int lora_rank,
                           void* packed, int dtype, void* stream) {
  MV_CHECK_ARG(params && dilations && packed && lora_rank > 0);
  MrfMeta meta;
  if (!mrf_make_meta(dilations, &meta)) return MV_ERR_UNSUPPORTED;
  if (dtype == MV_F32_W16) return mrf_pack_dispatch<f16>(params, meta, packed, lora_rank, param_dtype, (hipStream_t)stream);
  MV_DISPATCH(dtype, return mrf_pack_dispatch<T>(params, meta, packed, lora_rank, param_dtype, (hipStream_t)stream));
  return MV_OK;
}

// The block entry behind its name: argument checks, the instantiation per storage type, the launches - or, with `plan`, only what
// those launches would be (no HIP call).
static int mrf_block_run(const void* x, void* out, const void* packed, const int* dilations, void* workspace,
                         const uint8_t* dropout_mask, float mask_scale, int B, int T_, float eps, int dtype, void* stream,
                         MrfPlan* plan) {
  MV_CHECK_ARG(x && out && packed && dilations && workspace && B > 0 && B <= 65535 && T_ > 0 && x != out);
  MV_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)packed & 15) == 0);
  MrfMeta meta;
  if (!mrf_make_meta(dilations, &meta)) return MV_ERR_UNSUPPORTED;
  int rc;
  switch (dtype) {
    case MV_F32:
      // 8 waves x 16 steps (two waves per SIMD overlap each other's LDS / VALU phases: 150 -> 134 us per block at C2).  Where that
      // tile does not fit 160 KB next to the hi+lo weight images: 4 waves x 32 steps, same 128-step workgroup tile - with halos up
      // to MRF_HMAX = 8 it always fits (138176 + 576 x halo bytes, tests/test_host_mrf_plan.py), so the second line is never taken
      rc = mrf_launch<float, 8, 1>(x, out, packed, meta, (float*)workspace, dropout_mask, mask_scale, B, T_, eps, (hipStream_t)stream, plan);
      if (rc == MV_ERR_UNSUPPORTED)
        rc = mrf_launch<float, 4, 2>(x, out, packed, meta, (float*)workspace, dropout_mask, mask_scale, B, T_, eps, (hipStream_t)stream, plan);
      break;
    case MV_BF16: rc = mrf_launch<bf16, 8, 4>(x, out, packed, meta, (float*)workspace, dropout_mask, mask_scale, B, T_, eps, (hipStream_t)stream, plan); break;
    case MV_F16: rc = mrf_launch<f16, 8, 4>(x, out, packed, meta, (float*)workspace, dropout_mask, mask_scale, B, T_, eps, (hipStream_t)stream, plan); break;
    default: return MV_ERR_DTYPE;
  }
  if (rc != MV_OK || plan) return rc;
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_mrf_block_fwd_cl(const void* x, void* out, const void* packed, const int* dilations, void* workspace,
                                   const uint8_t* dropout_mask, float mask_scale, int B, int T_, float eps, int dtype,
                                   void* stream) {
  return mrf_block_run(x, out, packed, dilations, workspace, dropout_mask, mask_scale, B, T_, eps, dtype, stream, nullptr);
}

extern "C" size_t mv_mrf_chain_workspace_bytes(int B, int T_, int dtype) { return mrf_chain_ws(B, T_, dtype).total; }

// What both chain entries check and decode the same way, behind their own argument checks: pointers, alignment, one MrfMeta per block
// and the MV_F32_W16P code.  The dtype itself is judged by mrf_chain_run's switch, after the dilations.
static int mrf_chain_request(const void* x, void* out, const void* const* packed, const int* dilations, int nblocks, void* workspace,
                             int B, int T_, float eps, int dtype, void* stream, MrfChainReq* r) {
  MV_CHECK_ARG(x && packed && dilations && workspace && nblocks >= 1 && nblocks <= 8 && B > 0 && B <= 65535 && T_ > 0);
  MV_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 255) == 0);
  for (int i = 0; i < nblocks; ++i) {
    MV_CHECK_ARG(packed[i] && ((uintptr_t)packed[i] & 15) == 0);
    if (!mrf_make_meta(dilations + 3 * i, &r->metas[i])) return MV_ERR_UNSUPPORTED;
  }
  r->x = x; r->out = out; r->packed = packed; r->nblocks = nblocks; r->ws = (char*)workspace; r->B = B; r->T = T_; r->eps = eps;
  r->x_pair_in = dtype == MV_F32_W16P;
  r->dtype = r->x_pair_in ? MV_F32_W16 : dtype;
  r->stream = (hipStream_t)stream;
  return MV_OK;
}

// The one dispatcher of the chain: storage dtype -> form and tile geometry (see mrf_tile_t).  *tail is filled unless kind is MATERIALIZE.
static int mrf_chain_run(const MrfChainReq& r, MrfChainKind kind, MrfChainTail* tail, MrfPlan* plan = nullptr) {
  const MrfChainWs lay = mrf_chain_ws(r.B, r.T, r.dtype);
  int rc;
  switch (r.dtype) {
    case MV_F32:
      // as in the block entry: 4 waves x 32 steps where the 8 x 16 tile does not fit (never, with halos up to MRF_HMAX)
      rc = mrf_chain_launch<float, 8, 1>(r, lay, kind, tail, plan);
      if (rc == MV_ERR_UNSUPPORTED) rc = mrf_chain_launch<float, 4, 2>(r, lay, kind, tail, plan);
      break;
    case MV_F32_W16: {
      // every block with the dilations (1, 3, 5): the streaming form (mrf_stream.hip), else the tile form.  The streaming form has no
      // affine kernel (its tail goes to a consumer that takes the partial sums), and it alone reads pair-row input.
      bool all_std = true;
      for (int i = 0; i < r.nblocks; ++i) all_std = all_std && mrf_meta_is_std(r.metas[i]);
      if (all_std && kind != TAIL_WITH_AB) {
        rc = mvi_mrf_chain_stream(r.x, r.out, r.packed, r.nblocks, r.ws, lay, r.B, r.T, r.eps, r.stream, r.x_pair_in, tail, plan);
        if (plan && rc == MV_OK) { plan->kind = kind; plan->out_family = -1; plan->row_form = -1; }
        if (rc != MV_ERR_UNSUPPORTED) break;
      }
      if (r.x_pair_in) return MV_ERR_UNSUPPORTED;
      rc = mrf_chain_launch<f32w16, 8, 2>(r, lay, kind, tail, plan);
      break;
    }
    case MV_BF16: rc = mrf_chain_launch<bf16, 8, 4>(r, lay, kind, tail, plan); break;
    case MV_F16: rc = mrf_chain_launch<f16, 8, 4>(r, lay, kind, tail, plan); break;
    default: return MV_ERR_DTYPE;
  }
  if (rc != MV_OK || plan) return rc;
  MV_LAUNCH_CHECK();
  return MV_OK;
}

// chain + the generator's output projection (Conv1d(64,1,ks,pad ks/2) + activation): the last block's output is formed inside the
// output conv's staging loop and never stored
static int mrf_chain_out_run(const void* x, void* wave, const void* const* packed, const int* dilations, int nblocks,
                             void* workspace, const void* conv_packed, float conv_bias, int ks, int act, int B, int T_,
                             float eps, int dtype, void* stream, MrfPlan* plan) {
  MV_CHECK_ARG(wave && conv_packed && ks > 0 && (ks & 1));
  MrfChainReq r;
  int rc = mrf_chain_request(x, nullptr, packed, dilations, nblocks, workspace, B, T_, eps, dtype, stream, &r);
  if (rc != MV_OK) return rc;
  const int cdt = r.dtype == MV_F32_W16 ? MV_F32 : r.dtype;          // the output conv sees fp32 storage either way
  // the output conv forms the last block's affine itself where it can: one launch less
  const MrfChainKind kind = mvi_conv_out_affine_takes_partials(cdt, ks) ? TAIL_WITH_PARTIALS : TAIL_WITH_AB;
  MrfChainTail tail;
  rc = mrf_chain_run(r, kind, &tail, plan);
  if (rc != MV_OK) return rc;
  // conv_packed = mv_conv_out_pack_all image: the fp32 [ks][64] weights come first
  const float* ab = reinterpret_cast<const float*>(r.ws + mrf_chain_ws(B, T_, r.dtype).ab);
  rc = mvi_conv_out_affine(tail, ab, (const float*)conv_packed, conv_bias, wave, B, T_, MRF_C, ks, ks / 2, act, cdt, eps, r.stream, plan);
  if (rc != MV_OK || plan) return rc;
  MV_LAUNCH_CHECK();
  return MV_OK;
}

extern "C" int mv_mrf_chain_out_fwd_cl(const void* x, void* wave, const void* const* packed, const int* dilations, int nblocks,
                                       void* workspace, const void* conv_packed, float conv_bias, int ks, int act, int B, int T_,
                                       float eps, int dtype, void* stream) {
  return mrf_chain_out_run(x, wave, packed, dilations, nblocks, workspace, conv_packed, conv_bias, ks, act, B, T_, eps, dtype, stream,
                           nullptr);
}

// out == NULL: the chain's passes run and leave (f, x, partial sums) in the workspace, nothing is materialised (bench.py times the
// passes the generator really runs this way: its last block's output is formed inside the output conv)
static int mrf_chain_fwd_run(const void* x, void* out, const void* const* packed, const int* dilations, int nblocks,
                             void* workspace, int B, int T_, float eps, int dtype, void* stream, MrfPlan* plan) {
  MV_CHECK_ARG(((uintptr_t)out & 15) == 0);
  MrfChainReq r;
  const int rc = mrf_chain_request(x, out, packed, dilations, nblocks, workspace, B, T_, eps, dtype, stream, &r);
  if (rc != MV_OK) return rc;
  MrfChainTail tail;
  return mrf_chain_run(r, out ? MATERIALIZE : PASSES_ONLY, &tail, plan);
}

extern "C" int mv_mrf_chain_fwd_cl(const void* x, void* out, const void* const* packed, const int* dilations, int nblocks,
                                   void* workspace, int B, int T_, float eps, int dtype, void* stream) {
  return mrf_chain_fwd_run(x, out, packed, dilations, nblocks, workspace, B, T_, eps, dtype, stream, nullptr);
}

// The dry run of the four entries above for a geometry: the entry's return code for valid, aligned pointers and, for MV_OK, the plan
// (MrfPlan, in its field order).  Pure host code: the launchers return before their first HIP call when they are given a plan.
extern "C" int mv_mrf_plan(int entry, int B, int T_, int nblocks, const int* dilations, int dtype, int ks, int* out) {
  MV_CHECK_ARG(out && dilations && entry >= 0 && entry <= 3);
  alignas(256) static char dx[256], dy[256], dw[256], dp[256];     // stand-ins for valid pointers: compared and offset, never read
  const void* packs[8] = {dp, dp, dp, dp, dp, dp, dp, dp};
  MrfPlan plan = {};
  int rc;
  switch (entry) {
    case 0:
      MV_CHECK_ARG(nblocks == 1);
      rc = mrf_block_run(dx, dy, dp, dilations, dw, nullptr, 1.f, B, T_, 1e-5f, dtype, nullptr, &plan);
      break;
    case 1: rc = mrf_chain_fwd_run(dx, dy, packs, dilations, nblocks, dw, B, T_, 1e-5f, dtype, nullptr, &plan); break;
    case 2: rc = mrf_chain_fwd_run(dx, nullptr, packs, dilations, nblocks, dw, B, T_, 1e-5f, dtype, nullptr, &plan); break;
    default:
      rc = mrf_chain_out_run(dx, dy, packs, dilations, nblocks, dw, dp, 0.f, ks, MV_ACT_NONE, B, T_, 1e-5f, dtype, nullptr, &plan);
      break;
  }
  if (rc != MV_OK) return rc;
  const int v[20] = {plan.form, plan.nwaves, plan.ntw, plan.std_mask, plan.nwg, plan.nit, plan.wide, plan.tpw, plan.L, plan.lds,
                     plan.lds_wide, plan.lds_stat, plan.gx, plan.gy, plan.kind, plan.out_family, plan.row_form, plan.launches,
                     plan.hmax, plan.out_lds};
  for (int i = 0; i < 20; ++i) out[i] = v[i];
  return MV_OK;
}
