// PCEN front-end on the GPU (per-channel energy normalisation, Wang et al. 2017):
// AudioPreprocessor.compute_pcen (utils/manage_audio.py:28,44-47 of the reference), batched.
// PARITY UNPINNED: the reference's `pcen` package is absent; this is the published
// algorithm with the defaults of include/honk_hip.h.
//
//   pcm [B][S] f32 -> STFT as the MFCC's -> E[t][m] = sum_k melw[m][k] |X_t[k]|^power ->
//   M[0] = E[0], M[t] = (1 - s) M[t-1] + s E[t]   (per band, reset per clip) ->
//   out[t][m] = (E / (M + eps)^alpha + delta)^r - delta^r          [B][frames][n_mels] f32
//
// Fused route (the MFMA MFCC kernel's shapes): one workgroup per clip; the spectrum
// stage of mfcc_spectrum.h leaves E in LDS (its fixed-order mel accumulation: no float
// atomics, so a call gives the same bits on every run), the smoother and the compression
// run from there.
// Long route (every other shape): pcen_energy_kernel (direct DFT per (clip, FPB frames))
// writes E into out, pcen_scan_kernel turns out into PCEN in place.
//
// The smoother is a scan: M -> a M + b composes associatively, and a = 1 - s is the same
// at every step, so a segment of the time axis is summarised by its length and the b it
// leaves from M = 0.  A workgroup splits the time axis of its bands into segments, one
// thread per (band, segment): (1) each thread runs its segment from 0 (segment 0 from
// M[0] = E[0]); (2) one thread per band folds the summaries in order, M_end[j] =
// a^len_j M_end[j-1] + b_j; (3) each thread re-runs its segment from its carry, writing
// the compressed value over E.  Every element is read and written by one thread only.
#include "mfcc_spectrum.h"

#include <cmath>

namespace honk {
namespace pcen {

using mfcc::Args;
using mfcc::FPB;
using mfcc::MfmaArgs;

struct Params { float eps, s, alpha, delta, r; };

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

// ---- fused route ------------------------------------------------------------------ //
constexpr int FUSED_THREADS = 64 * mfcc::MF_WAVES;  // (front_plan: FUSED_THREADS / n_mels scan segments per band)

template <int POWER>
__global__ __launch_bounds__(FUSED_THREADS) void pcen_mfma_kernel(MfmaArgs ma, Params p, int nseg, int extra_off) {
  const Args& a = ma.a;
  extern __shared__ __attribute__((aligned(16))) float smf[];
  const int F = a.frames, NM = a.n_mels;
  // (the fixed-order mel accumulation: a call's output is the same bits on every run)
  float* melacc = mfcc::mfma_mel_energies<POWER, true>(ma, smf, smf + extra_off);
  scan_bands(melacc, F, NM, 0, NM, nseg, smf + extra_off + mfcc::ordered_floats(NM), p);
  __syncthreads();
  float* out = a.out + (int64_t)blockIdx.x * F * NM;
  for (int i = threadIdx.x; i < F * NM; i += blockDim.x) out[i] = melacc[i];
}

// ---- long route ------------------------------------------------------------------- //
template <int POWER>
__global__ __launch_bounds__(256) void pcen_energy_kernel(Args a) {
  extern __shared__ float sm[];
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * FPB;
  const int nf = min(FPB, a.frames - f0);
  const float* pw = mfcc::valu_spectrum<POWER>(a, sm, b, f0, nf);
  for (int q = threadIdx.x; q < nf * a.n_mels; q += blockDim.x) {
    const int f = q / a.n_mels, m = q - f * a.n_mels;
    const float* w = a.melw + (int64_t)m * a.n_bins;
    float s = 0.f;
    for (int k = 0; k < a.n_bins; ++k) s = fmaf(w[k], pw[f * a.n_bins + k], s);
    a.out[((int64_t)b * a.frames + f0 + f) * a.n_mels + m] = s;
  }
}

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_BANDS = 8;                          // bands per workgroup
constexpr int SCAN_SEGS = SCAN_THREADS / SCAN_BANDS;   // time segments per band

// grid (band groups, clips): out [B][F][NM] holds E on entry, PCEN on exit
__global__ __launch_bounds__(SCAN_THREADS) void pcen_scan_kernel(float* out, int F, int NM, Params p) {
  __shared__ float summ[SCAN_SEGS * SCAN_BANDS];
  const int band0 = blockIdx.x * SCAN_BANDS;
  const int nb = min(SCAN_BANDS, NM - band0);
  scan_bands(out + (int64_t)blockIdx.y * F * NM, F, NM, band0, nb, SCAN_SEGS, summ, p);
}

// route, frame count and LDS bytes come from front_plan (mfcc_spectrum.h), which honk_pcen_plan reports
template <int POWER>
static int launch(const Args& a, const mfcc::FrontPlan& fp, const Params& p, int64_t batch, hipStream_t stream) {
  const size_t lds = (size_t)fp.p.lds_bytes;
  if (fp.p.route == HONK_FRONT_ROUTE_MFMA) {
    MfmaArgs ma = fp.ma;
    ma.a = a;
    if (lds > mfcc::LDS_OPTIN)
      HONK_HIP_CHECK(hipFuncSetAttribute((const void*)pcen_mfma_kernel<POWER>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pcen_mfma_kernel<POWER>, dim3((unsigned)batch), dim3(FUSED_THREADS), lds, stream, ma, p, fp.nseg,
                       fp.extra_off);
    HONK_LAUNCH_CHECK("pcen_mfma_kernel");
    return HONK_OK;
  }
  hipLaunchKernelGGL(pcen_energy_kernel<POWER>, dim3((unsigned)cdiv(a.frames, FPB), (unsigned)batch), dim3(256), lds,
                     stream, a);
  HONK_LAUNCH_CHECK("pcen_energy_kernel");
  hipLaunchKernelGGL(pcen_scan_kernel, dim3((unsigned)cdiv(a.n_mels, SCAN_BANDS), (unsigned)batch),
                     dim3(SCAN_THREADS), 0, stream, a.out, a.frames, a.n_mels, p);
  HONK_LAUNCH_CHECK("pcen_scan_kernel");
  return HONK_OK;
}

}  // namespace pcen
}  // namespace honk

using namespace honk;

extern "C" int honk_pcen_plan(int32_t samples, int32_t n_fft, int32_t hop, int32_t n_mels, honk_front_plan_t* plan) {
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  mfcc::FrontPlan fp;
  const int rc = mfcc::front_plan(mfcc::FRONT_PCEN, samples, n_fft, hop, n_mels, n_mels, &fp);
  if (rc != HONK_OK) return rc;
  *plan = fp.p;
  return HONK_OK;
}

extern "C" int honk_pcen_f32(const float* pcm, int64_t batch, int32_t samples, const float* window, int32_t n_fft,
                             int32_t hop, const float* mel_weights, int32_t n_mels,
                             const honk_pcen_params_t* params, float* out, void* stream) {
  if (batch < 0) return fail(HONK_ERR_ARG, "bad pcen arguments");
  mfcc::FrontPlan fp;
  const int rc = mfcc::front_plan(mfcc::FRONT_PCEN, samples, n_fft, hop, n_mels, n_mels, &fp);
  if (rc != HONK_OK) return rc;
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
  if (batch == 0) return HONK_OK;
  if (!pcm || !window || !mel_weights || !out) return fail(HONK_ERR_ARG, "null pointer argument");
  if (batch > 65535) return fail(HONK_ERR_ARG, "batch > 65535 per call");
  mfcc::Args a;
  a.pcm = pcm; a.window = window; a.melw = mel_weights; a.dct = nullptr; a.out = out;
  a.S = samples; a.n_fft = n_fft; a.hop = hop; a.n_bins = fp.p.n_bins; a.n_mels = n_mels; a.n_dct = n_mels;
  a.frames = fp.p.frames;
  const pcen::Params p = {q.eps, q.s, q.alpha, q.delta, q.r};
  return q.power == 1 ? pcen::launch<1>(a, fp, p, batch, (hipStream_t)stream)
                      : pcen::launch<2>(a, fp, p, batch, (hipStream_t)stream);
}
