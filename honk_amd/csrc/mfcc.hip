// MFCC front-end on the GPU: AudioPreprocessor.compute_mfccs
// (/root/reference/utils/manage_audio.py:30-42, librosa 0.6 semantics), batched.
//
//   pcm [B][S] f32 (int16/32768) -> reflect-pad n_fft/2 -> frames (hop) ->
//   periodic Hann window -> |rDFT|^2 (n_fft/2+1 bins) -> mel filterbank ->
//   log of the positive entries -> DCT basis -> out [B][frames][n_dct] f32
//
// One workgroup per (clip, FPB frames): the padded samples of its frames are
// staged in LDS; each thread computes the power of some (frame, bin) pairs by a
// direct DFT with a twiddle table in LDS (n_fft = 480 is not a power of two;
// 23 MMAC/clip is far below the conv net behind it); mel + log + DCT follow in
// the same workgroup from LDS.  The mel and DCT matrices come from the host
// (honk_amd/audio.py builds them exactly as librosa 0.6 does).  The spectrum stage
// of both routes lives in mfcc_spectrum.h (the PCEN front end, pcen.hip, shares it).
#include "mfcc_spectrum.h"

namespace honk {
namespace mfcc {

__global__ __launch_bounds__(256) void mfcc_kernel(Args a) {
  extern __shared__ float sm[];
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * FPB;
  const int nf = min(FPB, a.frames - f0);
  float* pw = valu_spectrum<2>(a, sm, b, f0, nf);  // (mfcc_spectrum.h)
  float* lm = sm + valu_spectrum_floats(a.n_fft, a.hop, a.n_bins);  // [FPB][n_mels] log-mel
  // mel filterbank + log of positive entries (manage_audio.py:31-39)
  for (int q = threadIdx.x; q < nf * a.n_mels; q += blockDim.x) {
    const int f = q / a.n_mels, m = q - f * a.n_mels;
    const float* w = a.melw + (int64_t)m * a.n_bins;
    float s = 0.f;
    for (int k = 0; k < a.n_bins; ++k) s = fmaf(w[k], pw[f * a.n_bins + k], s);
    lm[f * a.n_mels + m] = s > 0.f ? logf(s) : s;
  }
  __syncthreads();
  // DCT (manage_audio.py:40): out[frame][i] = sum_m dct[i][m] * logmel[m]
  for (int q = threadIdx.x; q < nf * a.n_dct; q += blockDim.x) {
    const int f = q / a.n_dct, i = q - f * a.n_dct;
    const float* d = a.dct + (int64_t)i * a.n_mels;
    float s = 0.f;
    for (int m = 0; m < a.n_mels; ++m) s = fmaf(d[m], lm[f * a.n_mels + m], s);
    a.out[((int64_t)b * a.frames + f0 + f) * a.n_dct + i] = s;
  }
}


// MFMA path (the default when the shape allows it): mfma_mel_energies (mfcc_spectrum.h)
// leaves the clip's mel energies in LDS; log and the DCT run from there.
__global__ __launch_bounds__(64 * MF_WAVES) void mfcc_mfma_kernel(MfmaArgs ma) {
  const Args& a = ma.a;
  extern __shared__ __attribute__((aligned(16))) float smf[];
  const int F = a.frames, NM = a.n_mels;
  const int tid = threadIdx.x, b = blockIdx.x;
  float* melacc = mfma_mel_energies<2, false>(ma, smf);
  for (int i = tid; i < F * NM; i += blockDim.x) {
    const float v = melacc[i];
    melacc[i] = v > 0.f ? logf(v) : v;
  }
  __syncthreads();
  for (int q = tid; q < F * a.n_dct; q += blockDim.x) {
    const int f = q / a.n_dct, i = q - f * a.n_dct;
    const float* d = a.dct + (int64_t)i * NM;
    float acc = 0.f;
    for (int m = 0; m < NM; ++m) acc = fmaf(d[m], melacc[f * NM + m], acc);
    a.out[((int64_t)b * F + f) * a.n_dct + i] = acc;
  }
}

}  // namespace mfcc
}  // namespace honk

using namespace honk;

extern "C" int honk_mfcc_plan(int32_t samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_dct,
                              honk_front_plan_t* plan) {
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  mfcc::FrontPlan fp;
  const int rc = mfcc::front_plan(mfcc::FRONT_MFCC, samples, n_fft, hop, n_mels, n_dct, &fp);
  if (rc != HONK_OK) return rc;
  *plan = fp.p;
  return HONK_OK;
}

extern "C" int honk_mfcc_f32(const float* pcm, int64_t batch, int32_t samples, const float* window,
                             int32_t n_fft, int32_t hop, const float* mel_weights, int32_t n_mels,
                             const float* dct, int32_t n_dct, float* out, void* stream) {
  if (batch < 0) return fail(HONK_ERR_ARG, "bad mfcc arguments");
  // the shape checks, route, frame count and LDS bytes: front_plan (mfcc_spectrum.h), which honk_mfcc_plan reports
  mfcc::FrontPlan fp;
  const int rc = mfcc::front_plan(mfcc::FRONT_MFCC, samples, n_fft, hop, n_mels, n_dct, &fp);
  if (rc != HONK_OK) return rc;
  if (batch == 0) return HONK_OK;
  if (!pcm || !window || !mel_weights || !dct || !out) return fail(HONK_ERR_ARG, "null pointer argument");
  if (batch > 65535) return fail(HONK_ERR_ARG, "batch > 65535 per call");
  mfcc::Args a;
  a.pcm = pcm; a.window = window; a.melw = mel_weights; a.dct = dct; a.out = out;
  a.S = samples; a.n_fft = n_fft; a.hop = hop; a.n_bins = fp.p.n_bins; a.n_mels = n_mels; a.n_dct = n_dct;
  a.frames = fp.p.frames;
  const size_t lds = (size_t)fp.p.lds_bytes;
  if (fp.p.route == HONK_FRONT_ROUTE_MFMA) {
    fp.ma.a = a;
    if (lds > mfcc::LDS_OPTIN) HONK_HIP_CHECK(hipFuncSetAttribute((const void*)mfcc::mfcc_mfma_kernel,
                                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mfcc::mfcc_mfma_kernel, dim3((unsigned)batch), dim3(64 * mfcc::MF_WAVES), lds,
                       (hipStream_t)stream, fp.ma);
    HONK_LAUNCH_CHECK("mfcc_mfma_kernel");
    return HONK_OK;
  }
  dim3 grid((unsigned)cdiv(a.frames, mfcc::FPB), (unsigned)batch);
  hipLaunchKernelGGL(mfcc::mfcc_kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
  HONK_LAUNCH_CHECK("mfcc_kernel");
  return HONK_OK;
}
