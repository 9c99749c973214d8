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
// The smoother's segmented scan and the compression are pcen_scan.h's (shared with the
// strided-window call of mfcc_stream.hip).
#include "mfcc_spectrum.h"
#include "pcen_scan.h"

namespace honk {
namespace pcen {

using mfcc::Args;
using mfcc::FPB;
using mfcc::MfmaArgs;

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
  pcen::Params p;
  int power;
  const int prc = pcen::check_params(params, &p, &power);
  if (prc != HONK_OK) return prc;
  if (batch == 0) return HONK_OK;
  if (!pcm || !window || !mel_weights || !out) return fail(HONK_ERR_ARG, "null pointer argument");
  if (batch > 65535) return fail(HONK_ERR_ARG, "batch > 65535 per call");
  mfcc::Args a;
  a.pcm = pcm; a.window = window; a.melw = mel_weights; a.dct = nullptr; a.out = out;
  a.S = samples; a.n_fft = n_fft; a.hop = hop; a.n_bins = fp.p.n_bins; a.n_mels = n_mels; a.n_dct = n_mels;
  a.frames = fp.p.frames;
  return power == 1 ? pcen::launch<1>(a, fp, p, batch, (hipStream_t)stream)
                    : pcen::launch<2>(a, fp, p, batch, (hipStream_t)stream);
}
