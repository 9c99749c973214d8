// The spectrum stage of the audio front ends: a clip's STFT frames -> |X|^POWER -> mel
// energies in LDS.  Shared by the MFCC kernels (mfcc.hip: log + DCT follow) and the PCEN
// kernels (pcen.hip: smoother + root compression follow); POWER = 2 is the power
// spectrum the MFCC takes, POWER = 1 the magnitude sqrt(re^2 + im^2).
#pragma once
#include "common.h"

#include <cstdlib>

namespace honk {
namespace mfcc {

constexpr int FPB = 4;  // frames per workgroup (VALU route)

struct Args {
  const float* pcm;     // [B][S]
  const float* window;  // [n_fft]
  const float* melw;    // [n_mels][n_bins]
  const float* dct;     // [n_dct][n_mels]  (MFCC only)
  float* out;           // [B][frames][n_dct]
  int S, n_fft, hop, n_bins, n_mels, n_dct, frames;
};

__device__ __forceinline__ int reflect(int i, int n) {
  // numpy 'reflect' padding (no edge repeat), valid for |overhang| < n
  if (i < 0) return -i;
  if (i >= n) return 2 * n - 2 - i;
  return i;
}

template <int POWER>
__device__ __forceinline__ float spectrum_power(float re, float im) {
  const float p = re * re + im * im;
  return POWER == 2 ? p : sqrtf(p);
}

// floats of LDS the VALU spectrum stage takes (the caller's own buffers follow)
__host__ __device__ inline int valu_spectrum_floats(int n_fft, int hop, int n_bins) {
  return (FPB - 1) * hop + 3 * n_fft + FPB * n_bins;
}

// VALU route, one workgroup per (clip b, frames f0 .. f0 + nf): the padded samples of its
// frames are staged in LDS; each thread computes |X|^POWER of some (frame, bin) pairs by a
// direct DFT with a twiddle table in LDS.  Returns pw [FPB][n_bins] (in sm, synchronised).
template <int POWER>
__device__ __forceinline__ float* valu_spectrum(const Args& a, float* sm, int b, int f0, int nf) {
  const int pad = a.n_fft / 2;
  const int span = (FPB - 1) * a.hop + a.n_fft;
  float* xs = sm;                          // [span] windowless samples
  float* tw_c = xs + span;                 // [n_fft] cos(2 pi t / n_fft)
  float* tw_s = tw_c + a.n_fft;            // [n_fft] sin
  float* pw = tw_s + a.n_fft;              // [FPB][n_bins] power
  const float* x = a.pcm + (int64_t)b * a.S;
  for (int i = threadIdx.x; i < span; i += blockDim.x) {
    const int gi = f0 * a.hop + i - pad;
    xs[i] = (f0 * a.hop + i < a.S + 2 * pad) ? x[reflect(gi, a.S)] : 0.f;
  }
  for (int t = threadIdx.x; t < a.n_fft; t += blockDim.x) {
    float s, c;
    sincosf(6.283185307179586f * (float)t / (float)a.n_fft, &s, &c);
    tw_c[t] = c;
    tw_s[t] = s;
  }
  __syncthreads();
  // power spectrum: X_k = sum_n w[n] x[n] e^{-2 pi i k n / N}
  for (int q = threadIdx.x; q < nf * a.n_bins; q += blockDim.x) {
    const int f = q / a.n_bins, k = q - f * a.n_bins;
    const float* xf = xs + f * a.hop;
    float re = 0.f, im = 0.f;
    int idx = 0;
    for (int n = 0; n < a.n_fft; ++n) {
      const float v = xf[n] * a.window[n];
      re = fmaf(v, tw_c[idx], re);
      im = fmaf(v, tw_s[idx], im);
      idx += k;
      if (idx >= a.n_fft) idx -= a.n_fft;
    }
    pw[f * a.n_bins + k] = spectrum_power<POWER>(re, im);
  }
  __syncthreads();
  return pw;
}

// ---------------------------------------------------------------------------- //
// MFMA route (the default when the shape allows it): the spectrum of a clip's frames
// as one GEMM on v_mfma_f32_16x16x4_f32,
//     D[c][f] = sum_k T[c][k] * S[k][f],   S[k][f] = xpad[f*hop + k],
//     T[2b][k] = w[k] cos(2 pi b k / N),  T[2b+1][k] = -w[k] sin(2 pi b k / N),
// one workgroup per clip.  The padded signal lives in LDS (S fragments are 16-B
// reads of 4 consecutive samples); T fragments are built on the fly from a
// twiddle table + the window in LDS (index (b*k) mod N stepped incrementally),
// shared by all frame tiles of a column tile.  The accumulator layout gives each
// lane the (re, im) pairs of 2 bins of one frame, so |X|^2 needs no shuffles;
// |X|^POWER goes straight into the mel bins (LDS float atomics over each bin's
// nonzero mel range).
constexpr int MF_WAVES = 4;
constexpr int MF_MT = 7;  // frame tiles of 16 (frames <= 112)

struct MfmaArgs {
  Args a;
  int ntiles;  // column tiles of 16 (2 * n_bins columns, padded)
  int xp;      // floats of the padded signal image
};

// ---- the host's one route decision (honk_mfcc_f32, honk_pcen_f32 and their plan queries) ---- //
// frames of a centre-padded clip: n_fft/2 reflected samples on either side, so 1 + samples/hop
// for even n_fft; for odd n_fft the padded clip is one sample shorter than samples + n_fft
inline int centre_frames(int samples, int n_fft, int hop) {
  return (int)(1 + ((int64_t)samples + 2 * (n_fft / 2) - n_fft) / hop);
}

// ORDERED: the floats the fixed-order mel accumulation takes after the MFMA stage's own -- the
// |X|^POWER of one round of MF_WAVES column tiles [MF_MT*16][PW_STRIDE], then each band's
// bin range [n_mels]
constexpr int PW_STRIDE = 8 * MF_WAVES + 1;
__host__ __device__ inline int ordered_floats(int n_mels) { return MF_MT * 16 * PW_STRIDE + n_mels; }

enum Front { FRONT_MFCC = 0, FRONT_PCEN = 1 };
constexpr size_t LDS_OPTIN = 64 * 1024;   // above it a launch asks for the dynamic LDS first
constexpr size_t LDS_MFMA = 160 * 1024;   // the MFMA route's ceiling
constexpr size_t LDS_VALU = 64 * 1024;    // the VALU route's

struct FrontPlan {
  honk_front_plan_t p;  // what the plan queries report; p.lds_bytes is the main kernel's launch size
  MfmaArgs ma;          // MFMA route: ntiles, xp (ma.a is the caller's to fill)
  int nseg, extra_off;  // fused PCEN: scan segments per band, float offset of the ordered stage
};

// Route, frame count and LDS bytes of one front-end call; status and reason as the launch
// returns them.  Host-only, reads HONK_MFCC_VALU.  (PCEN: n_dct = n_mels.)
inline int front_plan(Front fe, int32_t samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_dct,
                      FrontPlan* fp) {
  const char* what = fe == FRONT_PCEN ? "pcen" : "mfcc";
  if (samples < 1 || n_fft < 2 || hop < 1 || n_mels < 1 || n_dct < 1) return fail(HONK_ERR_ARG, "bad %s arguments", what);
  if (n_fft / 2 >= samples) return fail(HONK_ERR_ARG, "reflect padding needs samples > n_fft/2");
  const int64_t n_bins = n_fft / 2 + 1;
  const int frames = centre_frames(samples, n_fft, hop);
  fp->p.frames = frames;
  fp->p.n_bins = (int32_t)n_bins;
  fp->nseg = 0;
  fp->extra_off = 0;
  // MFMA route: frames <= 112, n_fft and hop multiples of 16 / 4, its LDS plan fits
  if (frames <= MF_MT * 16 && n_fft % 16 == 0 && hop % 4 == 0 && !getenv("HONK_MFCC_VALU")) {
    size_t lds = sizeof(float) * ((size_t)(MF_MT * 16 - 1) * hop + 4 * (size_t)n_fft + (size_t)n_mels * n_bins +
                                  (size_t)MF_MT * 16 * n_mels) + sizeof(int) * (size_t)n_bins;
    int nseg = 0;
    size_t extra_off = 0;
    if (fe == FRONT_PCEN && lds <= LDS_MFMA) {  // the ordered mel stage and the scan's [nseg][n_mels] summaries
      nseg = n_mels >= 64 * MF_WAVES ? 1 : 64 * MF_WAVES / n_mels;
      extra_off = (lds + sizeof(float) - 1) / sizeof(float);
      lds = sizeof(float) * (extra_off + ordered_floats(n_mels) + (size_t)nseg * n_mels);
    }
    if (lds <= LDS_MFMA) {
      fp->nseg = nseg;
      fp->extra_off = (int)extra_off;
      fp->ma.ntiles = (int)cdiv(2 * n_bins, 16);
      fp->ma.xp = (MF_MT * 16 - 1) * hop + n_fft;  // floats of the padded signal image
      fp->p.route = HONK_FRONT_ROUTE_MFMA;
      fp->p.launches = 1;
      fp->p.lds_bytes = (int64_t)lds;
      return HONK_OK;
    }
  }
  // VALU route: the spectrum stage's floats (valu_spectrum_floats, in size_t), and the MFCC's
  // [FPB][n_mels] log-mel tile
  const size_t lds = sizeof(float) * ((size_t)(FPB - 1) * hop + 3 * (size_t)n_fft + FPB * (size_t)n_bins +
                                      (fe == FRONT_MFCC ? FPB * (size_t)n_mels : 0));
  if (lds > LDS_VALU) return fail(HONK_ERR_UNSUPPORTED, "%s: n_fft too large for the LDS plan", what);
  fp->p.route = HONK_FRONT_ROUTE_VALU;
  fp->p.launches = fe == FRONT_PCEN ? 2 : 1;
  fp->p.lds_bytes = (int64_t)lds;
  return HONK_OK;
}

// One column tile t of the GEMM for this wave: acc[m] = D[16 t + 4 g + r][16 m + i16].
__device__ __forceinline__ void mfma_tile(const Args& a, const float* xpad, const float* win, const float* tw, int t,
                                          int g, int i16, f32x4 (&acc)[MF_MT]) {
  const int N = a.n_fft, nkb = N / 16;
  // this lane's T row: column c = 16 t + i16 -> bin c/2, cos (even) / -sin (odd)
  const int c = 16 * t + i16;
  const int bin = c >> 1;
  const float* twp = tw + ((c & 1) ? N : 0);
  const int bstep = (int)(((int64_t)bin * 16) % N);
  const int bj = bin % N;
  int idx = (int)(((int64_t)bin * (4 * g)) % N);  // (bin * k) mod N at k = 16 kb + 4 g
#pragma unroll
  for (int m = 0; m < MF_MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = 16 * kb + 4 * g;
    float tv[4];
    int ij = idx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tv[j] = twp[ij] * win[k0 + j];
      ij += bj;
      if (ij >= N) ij -= N;
    }
    idx += bstep;
    if (idx >= N) idx -= N;
#pragma unroll
    for (int m = 0; m < MF_MT; ++m) {
      const f32x4 sv = *(const f32x4*)(xpad + (16 * m + i16) * a.hop + k0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[j], sv[j], acc[m], 0, 0, 0);
    }
  }
}

// Clip blockIdx.x's mel energies: returns melacc [MF_MT*16][n_mels] in smf (rows < frames
// valid), synchronised.  blockDim.x = 64 * MF_WAVES; smf holds front_plan's bytes.
// ORDERED = false: |X|^POWER goes straight into the mel bins by LDS float atomics (the
// order the waves arrive in: equal to rounding from run to run).  ORDERED = true: each
// round of MF_WAVES tiles parks |X|^POWER in `extra` (ordered_floats) and every (frame,
// band) sum is then extended by one thread in bin order: the same bits on every run.
template <int POWER, bool ORDERED>
__device__ __forceinline__ float* mfma_mel_energies(const MfmaArgs& ma, float* smf, float* extra = nullptr) {
  const Args& a = ma.a;
  const int N = a.n_fft, F = a.frames, NB = a.n_bins, NM = a.n_mels;
  float* xpad = smf;                  // [xp]
  float* win = xpad + ma.xp;          // [N]
  float* tw = win + N;                // [2N] cos | sin
  float* melw = tw + 2 * N;           // [NM][NB]
  float* melacc = melw + NM * NB;     // [MF_MT*16][NM]
  int* brange = (int*)(melacc + MF_MT * 16 * NM);  // [NB] first | last << 16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int b = blockIdx.x;
  const int pad = N / 2;
  const float* x = a.pcm + (int64_t)b * a.S;
  for (int i = tid; i < ma.xp; i += blockDim.x)
    xpad[i] = (i < a.S + 2 * pad) ? x[reflect(i - pad, a.S)] : 0.f;
  for (int t = tid; t < N; t += blockDim.x) {
    float sn, cs;
    sincosf(6.283185307179586f * (float)t / (float)N, &sn, &cs);
    win[t] = a.window[t];
    tw[t] = cs;
    tw[N + t] = -sn;
  }
  for (int i = tid; i < NM * NB; i += blockDim.x) melw[i] = a.melw[i];
  for (int i = tid; i < MF_MT * 16 * NM; i += blockDim.x) melacc[i] = 0.f;
  __syncthreads();
  if constexpr (!ORDERED) {
    for (int bb = tid; bb < NB; bb += blockDim.x) {
      int lo = NM, hi = -1;
      for (int m = 0; m < NM; ++m)
        if (melw[m * NB + bb] != 0.f) { lo = min(lo, m); hi = max(hi, m); }
      brange[bb] = (hi < lo) ? 0x7fff : (lo | (hi << 16));
    }
    __syncthreads();

    for (int t = wave; t < ma.ntiles; t += MF_WAVES) {
      f32x4 acc[MF_MT];
      mfma_tile(a, xpad, win, tw, t, g, i16, acc);
      // lane holds D[c = 16 t + 4 g + r][f = 16 m + i16]: bins 8 t + 2 g + {0, 1}
#pragma unroll
      for (int m = 0; m < MF_MT; ++m) {
        const int f = 16 * m + i16;
        if (f >= F) continue;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int bb = 8 * t + 2 * g + q;
          if (bb >= NB) continue;
          const float p = spectrum_power<POWER>(acc[m][2 * q], acc[m][2 * q + 1]);
          const int r = brange[bb];
          for (int mm = r & 0xffff; mm <= (r >> 16); ++mm) atomicAdd(&melacc[f * NM + mm], melw[mm * NB + bb] * p);
        }
      }
    }
    __syncthreads();
  } else {
    float* pwr = extra;                                   // [MF_MT*16][PW_STRIDE]
    int* mrange = (int*)(extra + MF_MT * 16 * PW_STRIDE);  // [NM] first | last << 16 nonzero bin
    for (int m = tid; m < NM; m += blockDim.x) {
      int lo = NB, hi = -1;
      for (int bb = 0; bb < NB; ++bb)
        if (melw[m * NB + bb] != 0.f) { lo = min(lo, bb); hi = max(hi, bb); }
      mrange[m] = (hi < lo) ? 0x7fff : (lo | (hi << 16));
    }
    __syncthreads();
    for (int t0 = 0; t0 < ma.ntiles; t0 += MF_WAVES) {
      const int t = t0 + wave;  // (wave-uniform)
      if (t < ma.ntiles) {
        f32x4 acc[MF_MT];
        mfma_tile(a, xpad, win, tw, t, g, i16, acc);
#pragma unroll
        for (int m = 0; m < MF_MT; ++m) {
          const int f = 16 * m + i16;
#pragma unroll
          for (int q = 0; q < 2; ++q)
            pwr[f * PW_STRIDE + 8 * wave + 2 * g + q] = spectrum_power<POWER>(acc[m][2 * q], acc[m][2 * q + 1]);
        }
      }
      __syncthreads();
      // bins [8 t0, 8 t0 + 8 MF_WAVES) of this round into every (frame, band) they reach; bins
      // >= NB (the padding columns, the tiles past ntiles) lie outside every band's range
      const int b0 = 8 * t0;
      for (int e = tid; e < F * NM; e += blockDim.x) {
        const int f = e / NM, mm = e - f * NM;
        const int r = mrange[mm];
        const int lo = max(r & 0xffff, b0), hi = min(r >> 16, b0 + 8 * MF_WAVES - 1);
        if (lo > hi) continue;
        float s = melacc[e];
        for (int bb = lo; bb <= hi; ++bb) s = fmaf(melw[mm * NB + bb], pwr[f * PW_STRIDE + bb - b0], s);
        melacc[e] = s;
      }
      __syncthreads();
    }
  }
  return melacc;
}

}  // namespace mfcc
}  // namespace honk
