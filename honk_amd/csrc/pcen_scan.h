// The part of PCEN after the mel energies, shared by honk_pcen_f32 (pcen.hip) and
// honk_pcen_windows_i16 (mfcc_stream.hip): parameter validation, the compression and
// the segmented scan of the smoother.
//
// The smoother is a scan: M -> a M + b composes associatively, and a = 1 - s is the same
// at every step, so a segment of the time axis is summarised by its length and the b it
// leaves from M = 0.  A workgroup splits the time axis of its bands into segments, one
// thread per (band, segment): (1) each thread runs its segment from 0 (segment 0 from
// M[0] = E[0]); (2) one thread per band folds the summaries in order, M_end[j] =
// a^len_j M_end[j-1] + b_j; (3) each thread re-runs its segment from its carry, writing
// the compressed value over E.  Every element is read and written by one thread only.
#pragma once
#include "common.h"

#include <cmath>

namespace honk {
namespace pcen {

struct Params { float eps, s, alpha, delta, r; };

// host-only: params (NULL: the HONK_PCEN_* defaults) -> *p and *power, or the status and
// reason both PCEN entry points give for a bad parameter
inline int check_params(const honk_pcen_params_t* params, Params* p, int* power) {
  honk_pcen_params_t q = {HONK_PCEN_EPS, HONK_PCEN_S, HONK_PCEN_ALPHA, HONK_PCEN_DELTA, HONK_PCEN_R, HONK_PCEN_POWER};
  if (params) q = *params;
  if (!std::isfinite(q.eps) || !std::isfinite(q.s) || !std::isfinite(q.alpha) || !std::isfinite(q.delta) ||
      !std::isfinite(q.r))
    return fail(HONK_ERR_ARG, "pcen: non-finite parameter");
  if (!(q.s > 0.f && q.s <= 1.f)) return fail(HONK_ERR_ARG, "pcen: s outside (0, 1]");
  if (!(q.eps > 0.f)) return fail(HONK_ERR_ARG, "pcen: eps <= 0");
  if (q.alpha < 0.f) return fail(HONK_ERR_ARG, "pcen: alpha < 0");
  if (q.delta < 0.f) return fail(HONK_ERR_ARG, "pcen: delta < 0");
  if (!(q.r > 0.f)) return fail(HONK_ERR_ARG, "pcen: r <= 0");
  if (q.power != 1 && q.power != 2) return fail(HONK_ERR_ARG, "pcen: power must be 1 or 2");
  *p = Params{q.eps, q.s, q.alpha, q.delta, q.r};
  *power = q.power;
  return HONK_OK;
}

// x^r for x >= 0, r > 0 (0 -> 0); the one expression both sides of the subtraction use
__device__ __forceinline__ float root(float x, float r) { return exp2f(r * log2f(x)); }

__device__ __forceinline__ float compress(float e, float m, const Params& p, float droot) {
  const float g = exp2f(-p.alpha * log2f(m + p.eps));  // m >= 0, eps > 0: a positive base
  const float t = e > 0.f ? e * g : 0.f;
  return root(t + p.delta, p.r) - droot;
}

// a^n by n multiplications (n <= a segment's length)
__device__ __forceinline__ float apow(float a, int n) {
  float v = 1.f;
  for (int i = 0; i < n; ++i) v *= a;
  return v;
}

// The segmented scan of bands [band0, band0 + nb) of one clip.  e: [F][stride] with E in
// and PCEN out (LDS or global), summ: LDS [nseg][nb].  Called by the whole workgroup.
__device__ __forceinline__ void scan_bands(float* e, int F, int stride, int band0, int nb, int nseg, float* summ,
                                           const Params& p) {
  const int L = (F + nseg - 1) / nseg;
  const float a = 1.f - p.s;
  const float droot = root(0.f + p.delta, p.r);
  for (int w = threadIdx.x; w < nb * nseg; w += blockDim.x) {
    const int seg = w / nb, bl = w - seg * nb;
    const int t0 = seg * L, t1 = min(F, t0 + L);
    const float* col = e + band0 + bl;
    float m = 0.f;
    int t = t0;
    if (seg == 0) { m = col[0]; t = 1; }  // M[0] = E[0]
    for (; t < t1; ++t) m = fmaf(a, m, p.s * col[(int64_t)t * stride]);
    summ[seg * nb + bl] = m;
  }
  __syncthreads();
  for (int bl = threadIdx.x; bl < nb; bl += blockDim.x) {
    const float aL = apow(a, L);
    float m = summ[bl];
    for (int seg = 1; seg < nseg; ++seg) {
      const int len = max(0, min(F, (seg + 1) * L) - seg * L);
      m = fmaf(len == L ? aL : apow(a, len), m, summ[seg * nb + bl]);
      summ[seg * nb + bl] = m;
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nb * nseg; w += blockDim.x) {
    const int seg = w / nb, bl = w - seg * nb;
    const int t0 = seg * L, t1 = min(F, t0 + L);
    float* col = e + band0 + bl;
    float m = seg ? summ[(seg - 1) * nb + bl] : 0.f;
    for (int t = t0; t < t1; ++t) {
      const float v = col[(int64_t)t * stride];
      m = t ? fmaf(a, m, p.s * v) : v;
      col[(int64_t)t * stride] = compress(v, m, p, droot);
    }
  }
}

}  // namespace pcen
}  // namespace honk
