// Device-side clip sampler: cut, resample, scale and noise a whole batch of training clips out of a device-resident corpus in one
// launch (mv_clip_gather; the arithmetic is defined in include/mi355x_vocoder.h).  configs/train_config.yaml:81-85 asks for
// pitch_shift, time_stretch and noise_level; one windowed-sinc resampling moves pitch and tempo together.
//
// One workgroup of 256 lanes per (clip, tile of 1024 output samples), four consecutive outputs per lane (one Philox call, one
// 16-byte store).  A resampled tile stages its source span (at most 2 * 1024 + 2 W + 1 samples, W = ceil(Z / c) <= 128) in LDS,
// decoded to fp32 and zero outside the utterance, and the filter table next to it when it fits; a copy tile reads the arena directly.
// The choice is per record, so uniform per workgroup.  No atomics, no communication between workgroups, plain vector stores.
#include "common.h"
#include "philox.h"

namespace mv {

struct ClipDesc {            // 48 bytes, mirrored by hifigan_modified/data.py CLIP_DESC
  long long src_off, src_len, pos_q32, rate_q32;
  float gain, noise_std;
  long long noise_ctr;
};
static_assert(sizeof(ClipDesc) == 48, "clip record layout");

constexpr int CLIP_TILE = 1024;                          // output samples per workgroup
constexpr int CLIP_LANES = 256;
constexpr int CLIP_PER = CLIP_TILE / CLIP_LANES;         // consecutive outputs per lane
constexpr int CLIP_WMAX = 128;                           // ceil(Z / c) at Z = 64, rate 2
constexpr int CLIP_SPAN = 2 * CLIP_TILE + 2 * CLIP_WMAX + 8;    // floats of LDS for the source span (a multiple of 4)
constexpr int CLIP_TAB_LDS_MAX = 12288;                  // table entries staged in LDS (48 KB); a longer table is read from global memory
constexpr long long CLIP_ONE = 1ll << 32;

template <int SRC> __device__ __forceinline__ float clip_src(const void* arena, long long idx);
template <> __device__ __forceinline__ float clip_src<0>(const void* arena, long long idx) { return static_cast<const float*>(arena)[idx]; }
template <> __device__ __forceinline__ float clip_src<1>(const void* arena, long long idx) {
  return (float)static_cast<const int16_t*>(arena)[idx] * 3.0517578125e-05f;      // q * 2^-15, exact
}

template <typename T> __device__ __forceinline__ void clip_store(T* p, const float* y, int n, bool vec) {
  if (vec && n == CLIP_PER) {
    if constexpr (std::is_same<T, float>::value) {
      *reinterpret_cast<float4*>(p) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
      alignas(8) T tmp[CLIP_PER];
#pragma unroll
      for (int e = 0; e < CLIP_PER; ++e) st<T>(tmp + e, y[e]);
      *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(tmp);
    }
  } else {
    for (int e = 0; e < n; ++e) st<T>(p + e, y[e]);
  }
}

template <typename T, int SRC, bool TAB_LDS>
__global__ __launch_bounds__(CLIP_LANES) void clip_gather_kernel(const void* __restrict__ arena, const ClipDesc* __restrict__ descs,
                                                                 const float* __restrict__ table, int Z, int P, T* __restrict__ wave,
                                                                 int T_, int ntiles, uint32_t k0, uint32_t k1) {
  extern __shared__ __attribute__((aligned(16))) float clip_sm[];
  float* xs = clip_sm;                       // [CLIP_SPAN] the tile's source span
  float* tl = clip_sm + CLIP_SPAN;           // [Z * P + 1] the table (TAB_LDS)
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles, tid = threadIdx.x;
  const ClipDesc d = descs[b];
  const int t0 = tile * CLIP_TILE;
  const int n = min(CLIP_TILE, T_ - t0);                 // outputs of this tile, >= 1
  const int t = t0 + tid * CLIP_PER;                     // this lane's first output
  const int nmine = min(CLIP_PER, T_ - t);               // <= 0: nothing to store
  long long rate = d.rate_q32;
  rate = rate < CLIP_ONE / 2 ? CLIP_ONE / 2 : (rate > 2 * CLIP_ONE ? 2 * CLIP_ONE : rate);
  const bool copy = rate == CLIP_ONE && (d.pos_q32 & 0xffffffffll) == 0;
  float s[CLIP_PER];

  if (copy) {
    const long long i0 = (d.pos_q32 >> 32) + t;
#pragma unroll
    for (int e = 0; e < CLIP_PER; ++e) {
      const long long j = i0 + e;
      s[e] = (e < nmine && j >= 0 && j < d.src_len) ? clip_src<SRC>(arena, d.src_off + j) : 0.f;
    }
  } else {
    // (unsigned products: a record is device data, and a wild position must wrap, not be undefined)
    const auto qof = [&](int tt) { return (long long)((unsigned long long)d.pos_q32 + (unsigned long long)tt * (unsigned long long)rate); };
    const long long big = rate > CLIP_ONE ? rate : CLIP_ONE;
    const int W = (int)(((long long)Z * big + CLIP_ONE - 1) >> 32);        // ceil(Z / c), <= 2 Z
    const long long i_first = qof(t0) >> 32, i_last = qof(t0 + n - 1) >> 32;
    const long long span_lo = i_first - W;
    long long span_ll = (i_last - i_first) + 2 * W + 2;
    const int span = (int)(span_ll < 0 ? 0 : (span_ll > CLIP_SPAN ? CLIP_SPAN : span_ll));
    for (int k = tid; k < span; k += CLIP_LANES) {
      const long long j = span_lo + k;
      xs[k] = (j >= 0 && j < d.src_len) ? clip_src<SRC>(arena, d.src_off + j) : 0.f;
    }
    const int ZP = Z * P;
    if (TAB_LDS)
      for (int k = tid; k <= ZP; k += CLIP_LANES) tl[k] = table[k];
    __syncthreads();
    const float* tab = TAB_LDS ? tl : table;
    const float c = fminf(1.f, 4294967296.f / (float)rate);
    const float Zf = (float)Z, Pf = (float)P;
    float fr[CLIP_PER], acc[CLIP_PER];
    int rel[CLIP_PER];
#pragma unroll
    for (int e = 0; e < CLIP_PER; ++e) {
      const long long q = qof(min(t + e, t0 + n - 1));                     // lanes past the end repeat the tile's last output
      fr[e] = (float)(uint32_t)(q & 0xffffffffll) * 2.3283064365386963e-10f;
      const long long r = (q >> 32) - i_first;
      rel[e] = (r < 0 || r > 2 * CLIP_TILE) ? 0 : (int)r;                  // (only a wrapped position can leave the span)
      acc[e] = 0.f;
    }
    const int ntap = 2 * W + 2;                                            // j = i - W .. i + W + 1, ascending
    for (int m = 0; m < ntap; ++m) {
      const float dm = (float)(m - W);
#pragma unroll
      for (int e = 0; e < CLIP_PER; ++e) {
        const float a = fabsf(dm - fr[e]) * c;
        const float u = a * Pf;
        const int k = min((int)u, ZP - 1);
        const float w = u - (float)k;
        const float h0 = tab[k], h1 = tab[k + 1];
        const float h = h0 + w * (h1 - h0);
        acc[e] += a <= Zf ? xs[rel[e] + m] * h : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < CLIP_PER; ++e) s[e] = c * acc[e];
  }

  if (nmine <= 0) return;
  float y[CLIP_PER];
#pragma unroll
  for (int e = 0; e < CLIP_PER; ++e) y[e] = d.gain * s[e];
  if (d.noise_std != 0.f) {
    const uint64_t blk = (uint64_t)(t / CLIP_PER), ctr = (uint64_t)d.noise_ctr;
    uint32_t r[4];
    philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32), k0, k1, r);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u1 = (float)((r[2 * h] >> 8) + 1u) * 5.9604644775390625e-08f;      // (0, 1]
      const float u2 = (float)(r[2 * h + 1] >> 8) * 5.9604644775390625e-08f;         // [0, 1)
      const float R = sqrtf(-2.f * logf(u1));
      y[2 * h] = fmaf(d.noise_std, R * cospif(2.f * u2), y[2 * h]);
      y[2 * h + 1] = fmaf(d.noise_std, R * sinpif(2.f * u2), y[2 * h + 1]);
    }
  }
  T* out = wave + (size_t)b * T_ + t;
  clip_store<T>(out, y, nmine, ((uintptr_t)out & (CLIP_PER * sizeof(T) - 1)) == 0);
}

}  // namespace mv

using namespace mv;

static_assert(CLIP_PER == 4, "one Philox call yields the four normals of a lane's outputs");

template <typename T, int SRC, bool TAB_LDS>
static void clip_launch(const void* arena, const void* descs, const float* table, int Z, int P, void* wave, int B, int T_, long key,
                        hipStream_t stream) {
  const int ntiles = cdiv(T_, CLIP_TILE);
  const size_t lds = (size_t)(CLIP_SPAN + (TAB_LDS ? (Z * P + 1 + 3) / 4 * 4 : 0)) * sizeof(float);
  hipLaunchKernelGGL((clip_gather_kernel<T, SRC, TAB_LDS>), dim3((unsigned)(B * ntiles)), dim3(CLIP_LANES), lds, stream, arena,
                     static_cast<const ClipDesc*>(descs), table, Z, P, static_cast<T*>(wave), T_, ntiles, (uint32_t)(uint64_t)key,
                     (uint32_t)((uint64_t)key >> 32));
}

extern "C" int mv_clip_gather(const void* arena, int src_kind, const void* descs_dev, const float* table, int Z, int P, void* wave,
                              int B, int Tn, long key, int dtype, void* stream) {
  MV_CHECK_ARG(arena && descs_dev && table && wave);
  MV_CHECK_ARG(src_kind == 0 || src_kind == 1);
  MV_CHECK_ARG(B >= 1 && Tn >= 1 && Tn <= (1 << 20));
  MV_CHECK_ARG(Z >= 1 && Z <= 64 && P >= 1 && P <= 1024);
  MV_CHECK_ARG(((uintptr_t)descs_dev & 7) == 0);
  MV_CHECK_ARG((long)B * cdiv(Tn, CLIP_TILE) <= 0x7fffffffl);             // one workgroup per (clip, tile) in a one-dimensional grid
  const bool tab_lds = Z * P + 1 <= CLIP_TAB_LDS_MAX;
  MV_DISPATCH(dtype, {
    if (src_kind == 0) {
      if (tab_lds) clip_launch<T, 0, true>(arena, descs_dev, table, Z, P, wave, B, Tn, key, (hipStream_t)stream);
      else clip_launch<T, 0, false>(arena, descs_dev, table, Z, P, wave, B, Tn, key, (hipStream_t)stream);
    } else {
      if (tab_lds) clip_launch<T, 1, true>(arena, descs_dev, table, Z, P, wave, B, Tn, key, (hipStream_t)stream);
      else clip_launch<T, 1, false>(arena, descs_dev, table, Z, P, wave, B, Tn, key, (hipStream_t)stream);
    }
  });
  MV_LAUNCH_CHECK();
  return MV_OK;
}
