// Strided-window MFCC of one long recording (the /listen front end): every window of
// `window` samples at stride `stride` of an int16 recording in device memory ->
// out [n_windows][frames][n_dct], the model input -- each STFT frame computed once.
//
// compute_mfccs reflect-pads every window on its own, so only the frames whose n_fft
// span crosses a window edge are window-specific (frames 0, 1, 99, 100 of the 101 at
// n_fft 480 / hop 160).  With stride % hop == 0 an interior frame f of window w is the
// global frame w * (stride / hop) + f of the recording, whichever window asks for it.
//
// One kernel, one workgroup per tile of FT frame slots.  A tile is made of groups: a
// group is a run of consecutive frames of one (real or virtual) window, staged in LDS
// as one contiguous reflected span of the recording (int16 -> fp32 * 2^-15, exact):
//   segment tiles  one group of FT frames: consecutive shared interior frames of the
//                  whole range (the "virtual window" from the first selected window's
//                  start to the last one's end, where no interior frame reflects), or,
//                  where windows leave gaps / on the unshared route, of one window;
//   edge tiles     FT / gs groups of gs slots: the head frames [0, flo) or the tail
//                  frames (fhi, frames) of one window, about that window's own bounds.
// The power spectrum is mfcc_mfma_kernel's GEMM (v_mfma_f32_16x16x4_f32, twiddle x
// window fragments built from LDS tables); a frame is one column of it, so its result
// depends on its own n_fft samples only, in a fixed order.  Power goes to an LDS tile;
// mel, log and DCT are fixed-order loops over that tile (no floating-point atomics);
// the finished frames are scattered from LDS to every (window, frame) that maps to them.
//
// PCEN over the same windows (honk_pcen_windows_i16): the kernel above with another
// epilogue, then a scan per window.  The mel energies E[f][m] of a frame are a function of
// its n_fft samples alone, so stage 1 stores each frame's E row ONCE (no fan-out): on the
// overlapping shared route into the workspace -- [G][n_mels] shared rows indexed by the
// virtual window's frame, then [n][head + tail][n_mels] edge rows -- and on the gapped and
// unshared routes, where every frame belongs to one window, straight into that window's
// rows of out.  Stage 2 (pcen_windows_scan_kernel, one workgroup per window) gathers the
// window's [frames][n_mels] tile into LDS, runs pcen_scan.h's segmented scan on it (M[0] =
// E[0] of the window's own reflected frame 0: the smoother restarts per window) and writes
// the window's rows of out once; the whole tile is read before any of it is written, so the
// in-place routes are safe.
//
// A batch of recordings of ragged length (honk_mfcc_segments_i16 / honk_pcen_segments_i16): the same
// kernels (SEG) over recordings concatenated in one buffer and located by offsets [n_rec + 1].  One
// route for the batch; the segment tiles of each recording laid out as above for that recording
// alone, in recording order; the edge tiles over the batch's global window index, so one edge tile
// holds windows of several recordings.  A workgroup (in an edge tile: each group) finds its recording
// by binary search over a per-recording table in device memory (struct Rec; filled on the host by the
// plan call), once, before staging, and keeps its groups in LDS.  out [sum W_r][frames][n_dct]: a
// recording's rows are, bit for bit, the single-recording call's -- the per-frame arithmetic is the
// same code.  PCEN: [sum G_r][n_mels] shared rows, then [sum W_r][head + tail][n_mels] edge rows in
// the workspace; stage 2 one workgroup per global window.
//
// Streams fed tick after tick (honk_mfcc_bank_tick_i16 / honk_pcen_bank_tick_i16): the same kernels
// (SRC_BANK) over "tail | chunk" of each fed stream, the tail and the finished rows the stream's next
// window reuses resident in a slot of caller memory between ticks; a row finished in one tick is, bit for
// bit, the row a later tick would compute, so a stream's rows over any chunking are the single-recording
// call's on the whole stream.  The layout and the hazard argument stand before bank_assemble_kernel.
#include <algorithm>
#include <vector>

#include "common.h"
#include "pcen_scan.h"

namespace honk {
namespace mfccs {

constexpr int WAVES = 4;
constexpr int MT = 2;        // frame tiles of 16 per workgroup
constexpr int FT = 16 * MT;  // frame slots per workgroup
constexpr int PADK = 8;      // floats inserted after every hop samples of a staged span: the slot stride is
                             // hop + 8 = 168 floats = 42 16-B slots.  A ds_read_b128 lane group is 8 frames at
                             // k-offset 4g and 8 at 4(g+1): 42 i mod 16 puts the first on the even slots of the
                             // 256-B bank row and the second on the odd ones (no conflict; hop alone is 4-way)
constexpr int MAX_MELS = 128;  // the mel-range table of the (fixed-size) workspace

enum { MODE_UNSHARED = 0, MODE_OVERLAP = 1, MODE_GAPPED = 2 };
// the epilogue of the frame-tile kernel: MFCC frames fanned out to their windows, or the mel
// energies of |X| (power 1) / |X|^2 (power 2), each frame's row stored once
enum { EPI_MFCC = 0, EPI_PCEN1 = 1, EPI_PCEN2 = 2 };
// where the frame-tile kernel's recordings lie: one recording (Args), a batch located by a table of Rec
// (honk_*_segments_i16), or the fed streams of a stream-bank tick located by a table of BankRec
// (honk_*_bank_tick_i16: "tail | chunk" assembled in the workspace, finished rows also kept in the slots)
enum { SRC_ONE = 0, SRC_SEG = 1, SRC_BANK = 2 };

// one row of the per-recording table of the batched calls (honk_*_segments_i16): filled on the host by
// the plan call, read on the device.  Row n_rec is a sentinel holding the totals, so the last r with
// tile0[r] <= t (window0[r] <= w) is the recording of tile t (window w) and never an empty one
struct Rec {
  int64_t tile0;    // first segment tile
  int64_t window0;  // first window: row of out
  int64_t srow0;    // first shared-frame row (MODE_OVERLAP)
  int64_t sample0;  // offsets[r]
  int64_t n;        // windows
  int64_t G;        // MODE_OVERLAP: shared frames
};

// one row of a stream-bank tick's table (honk_*_bank_tick_i16): the first six fields as Rec's, for the
// stream's "recording" of this tick -- tail | chunk, assembled in the workspace at sample0.  On the
// overlapping route the stream's virtual window starts with `cached` finished rows kept from earlier ticks:
// G counts only the frames jl >= flo + cached computed now, srow0 their first row
struct BankRec {
  int64_t tile0, window0, srow0, sample0, n, G;
  int64_t slot;       // the stream's slot of state_dev
  int64_t chunk0;     // chunk_offsets[r]
  int64_t chunk_len;  // new samples
  int64_t consumed;   // samples of tail | chunk the tick's windows use up: the new tail starts there
  int32_t tail;       // samples in the slot before the tick
  int32_t cached;     // rows of the slot's cache the tick reuses
  int32_t half;       // the cache half that holds them; the tick writes the other one
  int32_t new_tail;   // samples in the slot after the tick
};

// the slots of a stream bank: [tail_bytes of int16][2 halves of half_floats floats] each
struct BankGeo {
  char* state;
  int64_t slot_bytes, tail_bytes, half_floats;
  __host__ __device__ int16_t* tail(int64_t slot) const { return (int16_t*)(state + slot * slot_bytes); }
  __host__ __device__ float* cache(int64_t slot, int half) const {
    return (float*)(state + slot * slot_bytes + tail_bytes) + half * half_floats;
  }
};

struct Args {
  const int16_t* pcm;
  const float* window;  // [n_fft]
  const float* melw;    // [n_mels][n_bins]
  const float* dct;     // [n_dct][n_mels]
  const int* mrange;    // [n_mels][2] first, last nonzero bin of a mel row (workspace)
  float* out;           // [n][frames][n_dct]; PCEN epilogues: where the E rows go (header comment)
  int64_t first_sample;  // first_window * stride
  int64_t n;             // windows of the range
  int64_t G;             // MODE_OVERLAP: shared frames of the range
  int64_t seg_tiles;     // segment tiles; the edge tiles follow
  int stride, win_len, n_fft, hop, n_bins, n_mels, n_dct, frames;
  int flo, fhi;  // interior frames [flo, fhi] (flo > fhi: none)
  int mode, q;   // q = stride / hop (shared modes)
  int tps;       // per-window modes: segment tiles per window
  int gs, gpt, gspan;  // edge tiles: slots per group, groups per tile, LDS floats per group
  int xs_floats;
  // a batch of recordings (SEG kernels): n, G and seg_tiles are the batch's totals, first_sample is unused
  const Rec* table;  // [n_rec + 1]
  int64_t n_rec;
  // a stream-bank tick (SRC_BANK kernels): as a batch, the fed streams for recordings
  const BankRec* btable = nullptr;  // [n_rec + 1]
  BankGeo bank = {};
};

struct Group {
  int64_t base;  // sample of the (virtual) window's start
  int64_t L;     // its length: reflection bound
  int64_t wl;    // window (row block of out) of slot 0; MODE_OVERLAP segments: of the recording's first
  int64_t f0;    // frame of slot 0
  int64_t n;     // windows of the group's recording
  int64_t srow;  // MODE_OVERLAP: the recording's first shared-frame row
  int nf;        // frames (0: an empty group)
  // SRC_BANK, MODE_OVERLAP segments: a finished frame jl >= jc of the virtual window is also row jl - jc
  // of the slot's new cache (null: the bank keeps no rows)
  float* cnew;
  int64_t jc;
};

__device__ __forceinline__ int64_t reflect(int64_t i, int64_t n) {
  // numpy 'reflect' padding (no edge repeat), valid for |overhang| < n
  if (i < 0) return -i;
  if (i >= n) return 2 * n - 2 - i;
  return i;
}

// the last row r < n_rec of the table with tile0 (BY_TILE) / window0 <= v: log2(n_rec) steps
template <bool BY_TILE, class R>
__device__ __forceinline__ const R& rec_of(const R* table, int64_t n_rec, int64_t v) {
  int64_t lo = 0, hi = n_rec;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((BY_TILE ? table[mid].tile0 : table[mid].window0) <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return table[lo > 0 ? lo - 1 : 0];
}

template <int SRC>
__device__ __forceinline__ Group group_of(const Args& a, int64_t t, int gi) {
  Group g;
  g.cnew = nullptr;
  g.jc = 0;
  if (t < a.seg_tiles) {
    int64_t first = a.first_sample, n = a.n, G = a.G, w0 = 0, tl = t;
    int cached = 0;
    g.srow = 0;
    if constexpr (SRC == SRC_SEG) {
      const Rec& r = rec_of<true>(a.table, a.n_rec, t);
      first = r.sample0; n = r.n; G = r.G; w0 = r.window0; tl = t - r.tile0;
      g.srow = r.srow0;
    }
    if constexpr (SRC == SRC_BANK) {
      const BankRec& r = rec_of<true>(a.btable, a.n_rec, t);
      first = r.sample0; n = r.n; G = r.G; w0 = r.window0; tl = t - r.tile0;
      cached = r.cached;
      g.srow = r.srow0 - cached;  // (so that row srow + jl - flo is the computed frame jl's)
      if (a.mode == MODE_OVERLAP && a.bank.half_floats > 0) {
        g.cnew = a.bank.cache(r.slot, 1 - r.half);
        g.jc = n * a.q + a.flo;
      }
    }
    g.n = n;
    if (a.mode == MODE_OVERLAP) {
      g.base = first;
      g.L = (n - 1) * a.stride + a.win_len;
      g.wl = w0;
      g.f0 = a.flo + cached + tl * FT;
      g.nf = (int)min((int64_t)FT, G - tl * FT);
    } else {
      const int fa = a.mode == MODE_GAPPED ? a.flo : 0;
      const int fb = a.mode == MODE_GAPPED ? a.fhi + 1 : a.frames;
      const int64_t w = tl / a.tps;
      g.wl = w0 + w;
      g.base = first + w * a.stride;
      g.L = a.win_len;
      g.f0 = fa + (int)(tl % a.tps) * FT;
      g.nf = min(FT, fb - (int)g.f0);
    }
  } else {
    const int64_t gid = (t - a.seg_tiles) * a.gpt + gi;
    g.wl = gid >> 1;
    g.n = a.n;
    g.srow = 0;
    const bool live = g.wl < a.n && gi < a.gpt;
    g.base = a.first_sample + g.wl * a.stride;
    if constexpr (SRC == SRC_SEG) {
      g.base = 0;
      if (live) {
        const Rec& r = rec_of<false>(a.table, a.n_rec, g.wl);
        g.base = r.sample0 + (g.wl - r.window0) * a.stride;
      }
    }
    if constexpr (SRC == SRC_BANK) {
      g.base = 0;
      if (live) {
        const BankRec& r = rec_of<false>(a.btable, a.n_rec, g.wl);
        g.base = r.sample0 + (g.wl - r.window0) * a.stride;
      }
    }
    g.L = a.win_len;
    const bool tail = gid & 1;
    g.f0 = tail ? a.fhi + 1 : 0;
    g.nf = live ? (tail ? a.frames - 1 - a.fhi : a.flo) : 0;
  }
  return g;
}

// first / last bin with a nonzero weight of every mel row (last < first: an all-zero row);
// one wave per row
__global__ __launch_bounds__(64) void mel_range_kernel(const float* melw, int n_bins, int* mrange) {
  const int m = blockIdx.x;
  int lo = n_bins, hi = -1;
  for (int k = threadIdx.x; k < n_bins; k += 64)
    if (melw[(int64_t)m * n_bins + k] != 0.f) {
      lo = min(lo, k);
      hi = max(hi, k);
    }
  for (int o = 32; o; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
  }
  if (threadIdx.x == 0) {
    mrange[2 * m] = hi < 0 ? 0 : lo;
    mrange[2 * m + 1] = hi;
  }
}

// SEG: a batch of recordings -- every group finds its recording in a.table once (one lane per group,
// the groups kept in LDS behind the power tile), before staging
// SRC_BANK: the same over the fed streams of a tick, frames jl < flo + cached left to the cache kernel; a
// finished row the stream's next window reuses is stored to the slot's new cache half as well
template <int EPI, int SRC = SRC_ONE>
__global__ __launch_bounds__(64 * WAVES) void mfcc_windows_kernel(Args a) {
  constexpr bool SEG = SRC != SRC_ONE;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int N = a.n_fft, NB = a.n_bins, NM = a.n_mels, ND = a.n_dct, hop = a.hop, pad = N / 2;
  const int PS = NB | 1;            // odd row stride of the power tile
  float* xs = sm;                   // [xs_floats] staged spans; log-mel and output tiles later
  float* win = xs + a.xs_floats;    // [N]
  float* tw = win + N;              // [2N] cos | -sin
  float* pw = tw + 2 * N;           // [FT][PS] power
  float* lm = xs;                   // [FT][NM + 1] log-mel (after the GEMM)
  float* ot = lm + FT * (NM + 1);   // [FT][ND + 1] finished frames
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int64_t t = blockIdx.x;
  const bool edge = t >= a.seg_tiles;
  const int gs = edge ? a.gs : FT, ng = edge ? a.gpt : 1, gspan = edge ? a.gspan : 0;
  const int glen = (gs - 1) * hop + N;
  Group* grp = (Group*)(pw + FT * PS);  // [ng] (SEG; 8-byte aligned: every term before it is even)
  if constexpr (SEG) {
    if (tid < ng) grp[tid] = group_of<SRC>(a, t, tid);
    __syncthreads();
  }
  const auto group = [&](int gi) -> Group {
    if constexpr (SEG)
      return grp[gi];
    else
      return group_of<SRC_ONE>(a, t, gi);
  };

  for (int gi = 0; gi < ng; ++gi) {
    const Group gr = group(gi);
    const int have = gr.nf > 0 ? (gr.nf - 1) * hop + N : 0;
    const int64_t off0 = gr.f0 * hop - pad;
    float* xg = xs + gi * gspan;
    for (int i = tid; i < glen; i += blockDim.x) {
      float v = 0.f;
      if (i < have) v = (float)a.pcm[gr.base + reflect(off0 + i, gr.L)] * (1.f / 32768.f);
      xg[i + PADK * (i / hop)] = v;
    }
  }
  for (int k = tid; k < N; k += blockDim.x) {
    float sn, cs;
    sincosf(6.283185307179586f * (float)k / (float)N, &sn, &cs);
    win[k] = a.window[k];
    tw[k] = cs;
    tw[N + k] = -sn;
  }
  __syncthreads();

  // this lane's frame slots: 16 m + i16 -> LDS offset of the slot's first sample
  int soff[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int s = 16 * m + i16;
    const int gi = s / gs, fi = s - gi * gs;
    soff[m] = gi < ng ? gi * gspan + fi * (hop + PADK) : 0;
  }
  const int ntiles = (2 * NB + 15) / 16;
  const int nkb = N / 16;
  for (int ct = wave; ct < ntiles; ct += WAVES) {
    // this lane's T row: column c = 16 ct + i16 -> bin c/2, cos (even) / -sin (odd)
    const int c = 16 * ct + i16;
    const int bin = c >> 1;
    const float* twp = tw + ((c & 1) ? N : 0);
    const int bstep = (int)(((int64_t)bin * 16) % N);
    const int bj = bin % N;
    int idx = (int)(((int64_t)bin * (4 * g)) % N);  // (bin * k) mod N at k = 16 kb + 4 g
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
      const int k0 = 16 * kb + 4 * g;
      const int koff = k0 + PADK * ((16 * kb) / hop);  // hop % 16 == 0: a k-block stays in one hop
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
      for (int m = 0; m < MT; ++m) {
        const f32x4 sv = *(const f32x4*)(xs + soff[m] + koff);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[j], sv[j], acc[m], 0, 0, 0);
      }
    }
    // lane holds D[c = 16 ct + 4 g + r][slot 16 m + i16]: bins 8 ct + 2 g + {0, 1}
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const int bb = 8 * ct + 2 * g + qq;
        if (bb < NB) {
          float pv = acc[m][2 * qq] * acc[m][2 * qq] + acc[m][2 * qq + 1] * acc[m][2 * qq + 1];
          if constexpr (EPI == EPI_PCEN1) pv = sqrtf(pv);
          pw[(16 * m + i16) * PS + bb] = pv;
        }
      }
    }
  }
  __syncthreads();
  if constexpr (EPI != EPI_MFCC) {
    // E = mel x |X|^power over each row's nonzero bins, ascending; a frame's row leaves once, coalesced
    for (int e = tid; e < FT * NM; e += blockDim.x) {
      const int f = e % FT, m = e / FT;
      const float* w = a.melw + (int64_t)m * NB;
      const int lo = a.mrange[2 * m], hi = a.mrange[2 * m + 1];
      float s = 0.f;
      for (int k = lo; k <= hi; ++k) s = fmaf(w[k], pw[f * PS + k], s);
      lm[f * (NM + 1) + m] = s;
    }
    int64_t* erow = (int64_t*)(lm + FT * (NM + 1));  // [FT] the slot's row of a.out, -1: none (8-byte aligned)
    float** cdst = (float**)(erow + FT);             // [FT] SRC_BANK: the slot's row of the new cache, or null
    if (tid < FT) {
      const int gi = tid / gs, fi = tid - gi * gs;
      int64_t row = -1;
      float* keep = nullptr;
      if (gi < ng) {
        const Group gr = group(gi);
        if (fi < gr.nf) {
          if constexpr (SRC == SRC_BANK)
            if (!edge && gr.cnew && gr.f0 + fi >= gr.jc) keep = gr.cnew + (gr.f0 + fi - gr.jc) * NM;
          if (a.mode != MODE_OVERLAP)
            row = gr.wl * a.frames + gr.f0 + fi;
          else if (!edge)
            row = gr.srow + gr.f0 - a.flo + fi;
          else
            row = a.G + gr.wl * (a.flo + a.frames - 1 - a.fhi) + (gr.f0 > a.fhi ? a.flo : 0) + fi;
        }
      }
      erow[tid] = row;
      if constexpr (SRC == SRC_BANK) cdst[tid] = keep;
    }
    __syncthreads();
    for (int e = tid; e < FT * NM; e += blockDim.x) {
      const int s = e / NM, m = e - s * NM;
      if (erow[s] >= 0) a.out[erow[s] * NM + m] = lm[s * (NM + 1) + m];
      if constexpr (SRC == SRC_BANK)
        if (cdst[s]) cdst[s][m] = lm[s * (NM + 1) + m];
    }
    return;
  }
  // mel filterbank over each row's nonzero bins, ascending; log of the positive entries
  for (int e = tid; e < FT * NM; e += blockDim.x) {
    const int f = e % FT, m = e / FT;
    const float* w = a.melw + (int64_t)m * NB;
    const int lo = a.mrange[2 * m], hi = a.mrange[2 * m + 1];
    float s = 0.f;
    for (int k = lo; k <= hi; ++k) s = fmaf(w[k], pw[f * PS + k], s);
    lm[f * (NM + 1) + m] = s > 0.f ? logf(s) : s;
  }
  __syncthreads();
  for (int e = tid; e < FT * ND; e += blockDim.x) {
    const int f = e % FT, i = e / FT;
    const float* d = a.dct + (int64_t)i * NM;
    float s = 0.f;
    for (int m = 0; m < NM; ++m) s = fmaf(d[m], lm[f * (NM + 1) + m], s);
    ot[f * (ND + 1) + i] = s;
  }
  // where each slot goes: output rows row0 + d (frames - q), d < count -- window wl0 + d, frame f0 - d q
  int64_t* srow = (int64_t*)(ot + FT * (ND + 1));  // [FT] (8-byte aligned: FT is even)
  int* scnt = (int*)(srow + FT);                   // [FT]
  float** cdst = (float**)(scnt + FT);             // [FT] SRC_BANK: the slot's row of the new cache, or null
  const bool fan = !edge && a.mode == MODE_OVERLAP;
  if (tid < FT) {
    const int gi = tid / gs, fi = tid - gi * gs;
    int64_t row = 0;
    int cnt = 0;
    float* keep = nullptr;
    if (gi < ng) {
      const Group gr = group(gi);
      if (fi < gr.nf) {
        if (fan) {
          const int64_t jl = gr.f0 + fi;  // frame of the virtual window: frame jl - w q of window w
          if constexpr (SRC == SRC_BANK)
            if (gr.cnew && jl >= gr.jc) keep = gr.cnew + (jl - gr.jc) * ND;
          const int64_t wlo = jl > a.fhi ? (jl - a.fhi + a.q - 1) / a.q : 0;
          const int64_t whi = min(gr.n - 1, (jl - a.flo) / a.q);
          row = (gr.wl + wlo) * a.frames + (jl - wlo * a.q);
          cnt = (int)(whi - wlo + 1);
        } else {
          row = gr.wl * a.frames + gr.f0 + fi;
          cnt = 1;
        }
      }
    }
    srow[tid] = row;
    scnt[tid] = cnt;
    if constexpr (SRC == SRC_BANK) cdst[tid] = keep;
  }
  __syncthreads();
  const int cmax = fan ? (a.fhi - a.flo) / a.q + 1 : 1;
  const int per = cmax * ND;
  const int64_t rstep = fan ? a.frames - a.q : 0;
  for (int e = tid; e < FT * per; e += blockDim.x) {
    const int s = e / per, r = e - s * per;
    const int d = r / ND, i = r - d * ND;
    if (d < scnt[s]) a.out[(srow[s] + d * rstep) * ND + i] = ot[s * (ND + 1) + i];
  }
  if constexpr (SRC == SRC_BANK) {
    for (int e = tid; e < FT * ND; e += blockDim.x) {
      const int s = e / ND, i = e - s * ND;
      if (cdst[s]) cdst[s][i] = ot[s * (ND + 1) + i];
    }
  }
}

// ---- PCEN stage 2 -------------------------------------------------------------------- //
constexpr int SCAN_THREADS = 256;  // scan segments per band: SCAN_THREADS / n_mels (of the shape only)

struct ScanArgs {
  const float* e;  // MODE_OVERLAP: the workspace's E rows; else unused (E is in out)
  float* out;      // [n][frames][n_mels]
  int64_t G;
  int frames, n_mels, flo, fhi, q, mode, nseg;
  const Rec* table;  // a batch of recordings: G is the batch's total, w the global window; else null
  int64_t n_rec;
  // a stream-bank tick: G the tick's computed shared rows; an interior frame jl < flo + cached of a stream's
  // virtual window comes from the slot's old cache half, the others from e
  const BankRec* btable = nullptr;
  BankGeo bank = {};
};

// one workgroup per window: E tile -> LDS, smoother + compression there, the window's rows out
__global__ __launch_bounds__(SCAN_THREADS) void pcen_windows_scan_kernel(ScanArgs s, pcen::Params p) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [frames][n_mels], then summ [nseg][n_mels]
  const int F = s.frames, NM = s.n_mels;
  const int64_t w = blockIdx.x;
  float* o = s.out + w * F * NM;
  if (s.mode == MODE_OVERLAP) {
    const int ne = s.flo + F - 1 - s.fhi;
    int64_t srow = w * s.q - s.flo;
    if (s.table) {
      const Rec& r = rec_of<false>(s.table, s.n_rec, w);
      srow = r.srow0 + (w - r.window0) * s.q - s.flo;
    }
    const int64_t erow = s.G + w * ne;
    const float* old = nullptr;  // the stream's cached rows: frames [wq + flo, wq + flo + nold) of this window
    int64_t nold = 0;
    if (s.btable) {
      const BankRec& r = rec_of<false>(s.btable, s.n_rec, w);
      const int64_t wq = (w - r.window0) * s.q;
      srow = r.srow0 - r.cached + wq - s.flo;
      old = s.bank.cache(r.slot, r.half) + (wq - s.flo) * NM;
      nold = r.cached - wq;
    }
    for (int i = threadIdx.x; i < F * NM; i += blockDim.x) {
      const int f = i / NM, m = i - f * NM;
      const int64_t row = f < s.flo ? erow + f : (f > s.fhi ? erow + s.flo + (f - s.fhi - 1) : srow + f);
      const bool cached = f >= s.flo && f <= s.fhi && f - s.flo < nold;
      tile[i] = cached ? old[(int64_t)f * NM + m] : s.e[row * NM + m];
    }
  } else {
    for (int i = threadIdx.x; i < F * NM; i += blockDim.x) tile[i] = o[i];
  }
  __syncthreads();
  pcen::scan_bands(tile, F, NM, 0, NM, s.nseg, tile + F * NM, p);
  __syncthreads();
  for (int i = threadIdx.x; i < F * NM; i += blockDim.x) o[i] = tile[i];
}

struct Plan {
  honk_mfcc_windows_plan_t p;
  int flo, fhi, mode, q, gs;
};

// host-only; status and reason as the entry points return them
static int make_plan(int64_t samples, int32_t window, int32_t stride, int32_t n_fft, int32_t hop,
                     int64_t first_window, int64_t n_windows, Plan* pl) {
  if (samples < 0 || first_window < 0 || n_windows < 0) return fail(HONK_ERR_ARG, "negative count");
  if (stride < 1 || n_fft < 2 || hop < 1) return fail(HONK_ERR_ARG, "bad mfcc window arguments");
  if (window <= n_fft / 2) return fail(HONK_ERR_ARG, "reflect padding needs window > n_fft/2");
  const int64_t W = samples < window ? 0 : 1 + (samples - window) / stride;
  if (first_window > W || n_windows > W - first_window)
    return fail(HONK_ERR_ARG, "window range past the recording's %lld windows", (long long)W);
  if (n_fft % 16 || hop % 16) return fail(HONK_ERR_UNSUPPORTED, "mfcc windows: n_fft and hop must be multiples of 16");
  const int pad = n_fft / 2, frames = 1 + window / hop;
  pl->flo = (pad + hop - 1) / hop;
  pl->fhi = window >= pad ? (window - pad) / hop : -1;
  if (pl->fhi > frames - 1) pl->fhi = frames - 1;
  const int nint = pl->fhi - pl->flo + 1;
  const bool shared = stride % hop == 0 && nint > 0;
  pl->q = shared ? stride / hop : 0;
  pl->mode = !shared ? MODE_UNSHARED : (pl->q <= nint ? MODE_OVERLAP : MODE_GAPPED);
  const int nh = pl->flo, nt = frames - 1 - pl->fhi;
  pl->gs = nh > nt ? nh : nt;
  if (shared && pl->gs > FT) return fail(HONK_ERR_UNSUPPORTED, "mfcc windows: %d edge frames per side", pl->gs);
  honk_mfcc_windows_plan_t& p = pl->p;
  p.windows = W;
  p.frames = frames;
  p.shared = shared ? 1 : 0;
  if (!shared) {
    p.shared_frames = p.edge_frames = 0;
    p.frames_computed = n_windows * frames;
  } else {
    p.shared_frames = n_windows == 0 ? 0 : (pl->mode == MODE_OVERLAP ? (n_windows - 1) * pl->q + nint : n_windows * nint);
    p.edge_frames = n_windows * (frames - nint);
    p.frames_computed = p.shared_frames + p.edge_frames;
  }
  p.workspace_bytes = 2 * MAX_MELS * (int64_t)sizeof(int);
  return HONK_OK;
}

// host-only: the tiles and the LDS plan of the frame-tile kernel for a range (the shape fields of *a;
// the caller sets the pointers, n_mels and n_dct).  tail_floats: what the epilogue keeps in the span area
static int layout(const Plan& pl, const char* who, int32_t window, int32_t stride, int64_t first_window,
                  int64_t n_windows, int32_t n_fft, int32_t hop, int tail_floats, Args* ap, int64_t* tiles,
                  size_t* lds) {
  Args& a = *ap;
  a.first_sample = first_window * stride;
  a.n = n_windows;
  a.stride = stride; a.win_len = window; a.n_fft = n_fft; a.hop = hop; a.n_bins = n_fft / 2 + 1;
  a.frames = pl.p.frames;
  a.flo = pl.flo; a.fhi = pl.fhi; a.mode = pl.mode; a.q = pl.q;
  a.G = pl.p.shared_frames;
  a.tps = 1; a.gs = 1; a.gpt = 0; a.gspan = 0;
  a.table = nullptr; a.n_rec = 0;
  int64_t edge_tiles = 0;
  const int seg_floats = (FT - 1) * hop + n_fft + PADK * (FT + n_fft / hop);
  int xs = seg_floats;
  if (pl.mode == MODE_OVERLAP) {
    a.seg_tiles = cdiv(a.G, FT);
  } else {
    const int nfw = pl.mode == MODE_GAPPED ? pl.fhi - pl.flo + 1 : a.frames;
    a.tps = (int)cdiv(nfw, FT);
    a.seg_tiles = n_windows * a.tps;
  }
  if (pl.mode != MODE_UNSHARED && pl.gs > 0) {
    a.gs = pl.gs;
    a.gpt = FT / pl.gs;
    // floats of a group's padded span, rounded up to 16 mod 32: with gs = 2 the 8 groups of a lane
    // group's slots then fall on distinct slot pairs of the bank row, as the segment tiles' slots do
    int gspan = (pl.gs - 1) * hop + n_fft + PADK * (pl.gs + n_fft / hop);
    gspan = (gspan + 15) / 32 * 32 + 16;
    a.gspan = gspan;
    edge_tiles = cdiv(2 * n_windows, a.gpt);
    if (a.gpt * gspan > xs) xs = a.gpt * gspan;
  }
  if (tail_floats > xs) xs = tail_floats;
  a.xs_floats = (xs + 3) / 4 * 4;
  *tiles = a.seg_tiles + edge_tiles;
  *lds = sizeof(float) * ((size_t)a.xs_floats + 3 * (size_t)n_fft + (size_t)FT * (a.n_bins | 1));
  if (*lds > 160 * 1024) return fail(HONK_ERR_UNSUPPORTED, "%s windows: n_fft / hop too large for the LDS plan", who);
  if (*tiles > 0x7fffffff) return fail(HONK_ERR_UNSUPPORTED, "%s windows: too many frame tiles in one call", who);
  return HONK_OK;
}

// host-only: make_plan for the PCEN call -- the same counts, its own workspace (the mel-range table, then
// the E rows of the overlapping route) and stage 2's LDS plan
static int make_pcen_plan(int64_t samples, int32_t window, int32_t stride, int32_t n_fft, int32_t hop,
                          int32_t n_mels, int64_t first_window, int64_t n_windows, Plan* pl, int* nseg,
                          size_t* scan_lds) {
  if (n_mels < 1) return fail(HONK_ERR_ARG, "bad pcen arguments");
  const int rc = make_plan(samples, window, stride, n_fft, hop, first_window, n_windows, pl);
  if (rc != HONK_OK) return rc;
  if (n_mels > MAX_MELS) return fail(HONK_ERR_UNSUPPORTED, "pcen windows: more than %d mel bands", MAX_MELS);
  *nseg = SCAN_THREADS / n_mels;  // >= 2: n_mels <= 128
  *scan_lds = sizeof(float) * ((size_t)pl->p.frames + (size_t)*nseg) * (size_t)n_mels;
  if (*scan_lds > 160 * 1024)
    return fail(HONK_ERR_UNSUPPORTED, "pcen windows: a window's %d x %d tile past the LDS plan", pl->p.frames,
                n_mels);
  if (pl->mode == MODE_OVERLAP) pl->p.workspace_bytes += pl->p.frames_computed * n_mels * (int64_t)sizeof(float);
  return HONK_OK;
}

// ---- a batch of recordings ------------------------------------------------------------ //
struct SegPlan {
  honk_mfcc_segments_plan_t p;
  int64_t seg_tiles;  // sum over the recordings; the edge tiles (over the batch's windows) follow
};

// host-only: the batch's counts, window0 and the table from the offsets.  geo: make_plan's (make_pcen_plan's)
// route of the geometry, taken on a recording without windows; check_total: offsets[n_rec] against
// total_samples (the _i16 calls); e_floats: floats of E per computed frame the workspace holds (PCEN on
// the overlapping route, else 0)
static int make_segments_plan(const Plan& geo, const char* who, const int64_t* offsets, int64_t n_rec,
                              bool check_total, int64_t total_samples, int32_t window, int32_t stride,
                              int64_t e_floats, int64_t* window0, Rec* table, size_t table_capacity, SegPlan* sp) {
  if (n_rec < 0 || (check_total && total_samples < 0)) return fail(HONK_ERR_ARG, "negative count");
  if (!offsets) return fail(HONK_ERR_ARG, "null pointer argument");
  if (offsets[0] < 0) return fail(HONK_ERR_ARG, "%s segments: negative offset", who);
  for (int64_t r = 0; r < n_rec; ++r)
    if (offsets[r + 1] < offsets[r]) return fail(HONK_ERR_ARG, "%s segments: offsets decrease at recording %lld", who, (long long)r);
  if (check_total && offsets[n_rec] > total_samples)
    return fail(HONK_ERR_ARG, "%s segments: offsets run past the %lld samples", who, (long long)total_samples);
  honk_mfcc_segments_plan_t& p = sp->p;
  p = honk_mfcc_segments_plan_t{};
  p.frames = geo.p.frames;
  p.shared = geo.p.shared;
  p.table_bytes = (n_rec + 1) * (int64_t)sizeof(Rec);
  if (table && table_capacity < (size_t)p.table_bytes)
    return fail(HONK_ERR_WORKSPACE, "%s segments table: %zu bytes, %lld needed", who, table_capacity,
                (long long)p.table_bytes);
  const int nint = geo.fhi - geo.flo + 1;
  const int nfw = geo.mode == MODE_GAPPED ? nint : p.frames;  // per-window routes: segment frames of a window
  const int64_t tps = cdiv(nfw, FT);
  int64_t tiles = 0, windows = 0, srow = 0;
  for (int64_t r = 0; r < n_rec; ++r) {
    const int64_t len = offsets[r + 1] - offsets[r];
    const int64_t W = len < window ? 0 : 1 + (len - window) / stride;
    const int64_t G = geo.mode == MODE_OVERLAP && W > 0 ? (W - 1) * geo.q + nint : 0;
    if (window0) window0[r] = windows;
    if (table) table[r] = Rec{tiles, windows, srow, offsets[r], W, G};
    if (geo.mode == MODE_UNSHARED) {
      p.frames_computed += W * p.frames;
    } else {
      const int64_t shared = geo.mode == MODE_OVERLAP ? G : W * nint;
      p.shared_frames += shared;
      p.edge_frames += W * (p.frames - nint);
      srow += shared;
    }
    tiles += geo.mode == MODE_OVERLAP ? cdiv(G, FT) : W * tps;
    windows += W;
  }
  if (geo.mode != MODE_UNSHARED) p.frames_computed = p.shared_frames + p.edge_frames;
  if (window0) window0[n_rec] = windows;
  if (table) table[n_rec] = Rec{tiles, windows, srow, offsets[n_rec], 0, 0};
  sp->seg_tiles = tiles;
  if (geo.mode != MODE_UNSHARED && geo.gs > 0) tiles += cdiv(2 * windows, FT / geo.gs);
  p.windows = windows;
  p.tiles = tiles;
  p.workspace_bytes = 2 * MAX_MELS * (int64_t)sizeof(int) + p.frames_computed * e_floats * (int64_t)sizeof(float);
  if (tiles > 0x7fffffff) return fail(HONK_ERR_UNSUPPORTED, "%s segments: too many frame tiles in one call", who);
  return HONK_OK;
}

// host-only: layout()'s shape fields and LDS plan for the batch (the groups' table behind the power tile)
static int segments_layout(const Plan& geo, const SegPlan& sp, const char* who, int32_t window, int32_t stride,
                           int32_t n_fft, int32_t hop, int tail_floats, const void* table_dev, int64_t n_rec,
                           Args* ap, size_t* lds) {
  int64_t none;
  const int rc = layout(geo, who, window, stride, 0, 0, n_fft, hop, tail_floats, ap, &none, lds);
  if (rc != HONK_OK) return rc;
  ap->n = sp.p.windows;
  ap->G = sp.p.shared_frames;
  ap->seg_tiles = sp.seg_tiles;
  ap->table = (const Rec*)table_dev;
  ap->n_rec = n_rec;
  *lds += FT * sizeof(Group);
  if (*lds > 160 * 1024) return fail(HONK_ERR_UNSUPPORTED, "%s segments: n_fft / hop too large for the LDS plan", who);
  return HONK_OK;
}

// ---- a stream bank: tails and finished rows resident between ticks ---------------------- //
// A slot of state_dev is [tail: the stream's unconsumed samples][two cache halves of cache_rows rows].  A
// tick is a chain of launches on one stream; within a launch no location is read by one workgroup and
// written by another:
//   bank_assemble_kernel  slot tails, chunks_dev -> "tail | chunk" per fed stream in the workspace
//   mfcc_windows_kernel   <SRC_BANK> workspace -> out (PCEN: E rows in the workspace), the new cache half
//   pcen_windows_scan     (PCEN) old cache half, workspace -> out
//   bank_cache_kernel     old cache half -> out (MFCC), the new cache half
//   bank_tail_kernel      workspace -> slot tails
// The old and the new cache of a slot are different halves (the host's parity bit flips when a tick
// completes a window), and the tail goes through the workspace, so no launch updates anything in place.
constexpr int BANK_THREADS = 256;
constexpr int BANK_MAX_Y = 64;  // workgroups along a stream's samples in the two copy kernels

__global__ __launch_bounds__(BANK_THREADS) void bank_assemble_kernel(const BankRec* table, BankGeo bank,
                                                                     const int16_t* chunks, int16_t* pcm) {
  const BankRec r = table[blockIdx.x];
  const int16_t* tail = bank.tail(r.slot);
  const int64_t len = r.tail + r.chunk_len;
  for (int64_t i = (int64_t)blockIdx.y * BANK_THREADS + threadIdx.x; i < len; i += (int64_t)gridDim.y * BANK_THREADS)
    pcm[r.sample0 + i] = i < r.tail ? tail[i] : chunks[r.chunk0 + (i - r.tail)];
}

__global__ __launch_bounds__(BANK_THREADS) void bank_tail_kernel(const BankRec* table, BankGeo bank,
                                                                 const int16_t* pcm) {
  const BankRec r = table[blockIdx.x];
  int16_t* tail = bank.tail(r.slot);
  const int16_t* src = pcm + r.sample0 + r.consumed;
  for (int i = blockIdx.y * BANK_THREADS + threadIdx.x; i < r.new_tail; i += gridDim.y * BANK_THREADS)
    tail[i] = src[i];
}

// the cached rows of a fed stream that completes n >= 1 windows, FT rows per workgroup (blockIdx.y): row i
// is frame jl = flo + i of the stream's virtual window.  MFCC (out != null): the fan-out of the frame-tile
// kernel for that frame -- frame jl - d q of window d, d <= min(n - 1, i / q); jl <= fhi - q, so d starts at
// 0.  A row i >= n q is row i - n q of the new cache (the frames the tick computes fill the rest)
__global__ __launch_bounds__(BANK_THREADS) void bank_cache_kernel(const BankRec* table, BankGeo bank, float* out,
                                                                  int cols, int frames, int flo, int q) {
  const BankRec r = table[blockIdx.x];
  const int row0 = blockIdx.y * FT;
  if (r.n < 1 || row0 >= r.cached) return;
  const int rows = min(FT, r.cached - row0);
  const float* old = bank.cache(r.slot, r.half);
  float* fresh = bank.cache(r.slot, 1 - r.half);
  for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
    const int i = row0 + e / cols, c = e % cols;
    const float v = old[(int64_t)i * cols + c];
    if (out) {
      const int64_t dmax = min(r.n - 1, (int64_t)(i / q));
      for (int64_t d = 0; d <= dmax; ++d) out[((r.window0 + d) * frames + (flo + i - d * q)) * cols + c] = v;
    }
    if (i >= r.n * q) fresh[(int64_t)(i - r.n * q) * cols + c] = v;
  }
}

struct BankPlan {
  honk_stream_bank_plan_t p;
  BankGeo geo;  // (state null)
};

// host-only: the slot layout of a geometry (geo: make_plan's route on a recording without windows)
static void make_bank_plan(const Plan& geo, int32_t window, int32_t row_floats, BankPlan* bp) {
  honk_stream_bank_plan_t& p = bp->p;
  p = honk_stream_bank_plan_t{};
  const int nint = geo.fhi - geo.flo + 1;
  p.tail_capacity = window - 1;
  p.cache_rows = geo.mode == MODE_OVERLAP ? nint - geo.q : 0;
  p.route = geo.mode;
  p.frames = geo.p.frames;
  p.row_floats = row_floats;
  p.flo = geo.flo; p.fhi = geo.fhi; p.q = geo.q;
  bp->geo.state = nullptr;
  bp->geo.tail_bytes = (2 * (int64_t)p.tail_capacity + 15) / 16 * 16;
  bp->geo.half_floats = (int64_t)p.cache_rows * row_floats;
  bp->geo.slot_bytes = (bp->geo.tail_bytes + 2 * bp->geo.half_floats * (int64_t)sizeof(float) + 15) / 16 * 16;
  p.slot_bytes = bp->geo.slot_bytes;
}

struct TickPlan {
  honk_bank_tick_plan_t p;
  int64_t seg_tiles, shared_rows, pcm_offset, max_len;
};

// host-only: a tick's counts, window0, the next state of the fed slots and the table.  e_floats as
// make_segments_plan's.  Nothing is written unless the whole tick is accepted
static int make_tick_plan(const Plan& geo, const BankPlan& bank, const char* who, const honk_bank_slot_t* slots,
                          int64_t n_slots, const int64_t* slot_ids, const int64_t* offsets, int64_t n_fed,
                          int32_t window, int32_t stride, int64_t e_floats, int64_t* window0, honk_bank_slot_t* next,
                          BankRec* table, size_t table_capacity, TickPlan* tp) {
  if (n_slots < 0 || n_fed < 0) return fail(HONK_ERR_ARG, "negative count");
  if (!offsets || (n_fed > 0 && (!slots || !slot_ids))) return fail(HONK_ERR_ARG, "null pointer argument");
  if (offsets[0] < 0) return fail(HONK_ERR_ARG, "%s bank tick: negative offset", who);
  for (int64_t r = 0; r < n_fed; ++r)
    if (offsets[r + 1] < offsets[r])
      return fail(HONK_ERR_ARG, "%s bank tick: offsets decrease at stream %lld", who, (long long)r);
  honk_bank_tick_plan_t& p = tp->p;
  p = honk_bank_tick_plan_t{};
  p.table_bytes = (n_fed + 1) * (int64_t)sizeof(BankRec);
  if (table && table_capacity < (size_t)p.table_bytes)
    return fail(HONK_ERR_WORKSPACE, "%s bank tick table: %zu bytes, %lld needed", who, table_capacity,
                (long long)p.table_bytes);
  static thread_local std::vector<uint8_t> fed;  // (host bookkeeping of the plan; nothing on the device)
  fed.assign((size_t)n_slots, 0);
  const int rows = bank.p.cache_rows;
  for (int64_t r = 0; r < n_fed; ++r) {
    const int64_t id = slot_ids[r];
    if (id < 0 || id >= n_slots)
      return fail(HONK_ERR_ARG, "%s bank tick: slot %lld of %lld", who, (long long)id, (long long)n_slots);
    if (fed[(size_t)id]) return fail(HONK_ERR_ARG, "%s bank tick: slot %lld fed twice", who, (long long)id);
    fed[(size_t)id] = 1;
    const honk_bank_slot_t& s = slots[id];
    if (s.tail < 0 || s.tail > bank.p.tail_capacity || (s.cached != 0 && s.cached != rows) || s.skip < 0 ||
        (s.skip > 0 && s.tail > 0) || (s.parity != 0 && s.parity != 1))
      return fail(HONK_ERR_ARG, "%s bank tick: slot %lld holds no valid state", who, (long long)id);
    if (s.skip > 0 && offsets[r + 1] > offsets[r])
      return fail(HONK_ERR_ARG, "%s bank tick: slot %lld still skips %d samples (stride > window): the caller "
                  "drops them before the upload", who, (long long)id, s.skip);
  }
  const int nint = geo.fhi - geo.flo + 1;
  const int nfw = geo.mode == MODE_GAPPED ? nint : geo.p.frames;
  const int64_t tps = cdiv(nfw, FT);
  int64_t tiles = 0, windows = 0, srow = 0, pos = 0, max_len = 0;
  for (int64_t r = 0; r < n_fed; ++r) {
    const honk_bank_slot_t& s = slots[slot_ids[r]];
    const int64_t c = offsets[r + 1] - offsets[r], len = s.tail + c;
    const int64_t n = len < window ? 0 : 1 + (len - window) / stride;
    const int64_t consumed = n * stride < len ? n * stride : len;
    const int cached = geo.mode == MODE_OVERLAP ? s.cached : 0;
    const int64_t G = geo.mode == MODE_OVERLAP && n > 0 ? (n - 1) * geo.q + nint - cached : 0;
    honk_bank_slot_t nx = s;
    nx.tail = (int32_t)(len - consumed);
    if (n > 0) {
      nx.skip = (int32_t)(n * stride - consumed);
      nx.cached = rows;
      if (rows > 0) nx.parity = 1 - s.parity;
    }
    if (window0) window0[r] = windows;
    if (next) next[r] = nx;
    if (table)
      table[r] = BankRec{tiles, windows, srow, pos, n, G, slot_ids[r], offsets[r], c, consumed, s.tail, cached,
                         s.parity, nx.tail};
    if (geo.mode == MODE_UNSHARED) {
      p.frames_computed += n * geo.p.frames;
    } else {
      const int64_t shared = geo.mode == MODE_OVERLAP ? G : n * nint;
      srow += shared;
      p.edge_frames += n * (geo.p.frames - nint);
      p.frames_computed += shared + n * (geo.p.frames - nint);
      if (n > 0) p.frames_reused += cached;
    }
    tiles += geo.mode == MODE_OVERLAP ? cdiv(G, FT) : n * tps;
    windows += n;
    pos += len;
    if (len > max_len) max_len = len;
  }
  if (window0) window0[n_fed] = windows;
  if (table) table[n_fed] = BankRec{tiles, windows, srow, pos, 0, 0, 0, offsets[n_fed], 0, 0, 0, 0, 0, 0};
  tp->seg_tiles = tiles;
  tp->shared_rows = srow;
  tp->max_len = max_len;
  if (geo.mode != MODE_UNSHARED && geo.gs > 0) tiles += cdiv(2 * windows, FT / geo.gs);
  p.windows = windows;
  p.tiles = tiles;
  p.samples_in = offsets[n_fed] - offsets[0];
  tp->pcm_offset = (2 * MAX_MELS * (int64_t)sizeof(int) + p.frames_computed * e_floats * (int64_t)sizeof(float) + 15) /
                   16 * 16;
  p.workspace_bytes = tp->pcm_offset + 2 * pos;
  if (tiles > 0x7fffffff || windows > 0x7fffffff || n_fed > 0x7fffffff)
    return fail(HONK_ERR_UNSUPPORTED, "%s bank tick: too many frame tiles in one call", who);
  return HONK_OK;
}

// host-only: the shape checks of both front ends' bank calls -> the route, the slot layout, stage 2's plan
static int bank_geometry(bool pcen, int32_t window, int32_t stride, int32_t n_fft, int32_t hop, int32_t row_floats,
                         Plan* geo, BankPlan* bank, int* nseg, size_t* scan_lds) {
  if (row_floats < 1) return fail(HONK_ERR_ARG, pcen ? "bad pcen arguments" : "bad mfcc arguments");
  const int rc = pcen ? make_pcen_plan(0, window, stride, n_fft, hop, row_floats, 0, 0, geo, nseg, scan_lds)
                      : make_plan(0, window, stride, n_fft, hop, 0, 0, geo);
  if (rc != HONK_OK) return rc;
  make_bank_plan(*geo, window, row_floats, bank);
  return HONK_OK;
}

static int bank_tick_plan(bool pcen, const honk_bank_slot_t* slots, int64_t n_slots, const int64_t* slot_ids,
                          const int64_t* offsets, int64_t n_fed, int32_t window, int32_t stride, int32_t n_fft,
                          int32_t hop, int32_t row_floats, int64_t* window0, honk_bank_slot_t* next, void* table,
                          size_t table_capacity, honk_bank_tick_plan_t* plan) {
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  Plan geo;
  BankPlan bank;
  int nseg;
  size_t scan_lds;
  const int rc = bank_geometry(pcen, window, stride, n_fft, hop, row_floats, &geo, &bank, &nseg, &scan_lds);
  if (rc != HONK_OK) return rc;
  TickPlan tp;
  const int trc = make_tick_plan(geo, bank, pcen ? "pcen" : "mfcc", slots, n_slots, slot_ids, offsets, n_fed, window,
                                 stride, pcen && geo.mode == MODE_OVERLAP ? row_floats : 0, window0, next,
                                 (BankRec*)table, table_capacity, &tp);
  if (trc != HONK_OK) return trc;
  *plan = tp.p;
  return HONK_OK;
}

// the tick of either front end: params null: MFCC (cols = n_dct), else PCEN (cols = n_mels)
static int bank_tick(const honk_pcen_params_t* params, bool pcen, const int16_t* chunks_dev,
                     const honk_bank_slot_t* slots, int64_t n_slots, const int64_t* slot_ids, const int64_t* offsets,
                     int64_t n_fed, const void* table_dev, size_t table_bytes, void* state_dev, size_t state_bytes,
                     int32_t window, int32_t stride, const float* window_tbl, int32_t n_fft, int32_t hop,
                     const float* mel_weights, int32_t n_mels, const float* dct, int32_t n_dct, float* out,
                     void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = pcen ? "pcen" : "mfcc";
  if (!pcen && (n_mels < 1 || n_dct < 1)) return fail(HONK_ERR_ARG, "bad mfcc arguments");
  const int cols = pcen ? n_mels : n_dct;
  Plan geo;
  BankPlan bank;
  ScanArgs sa;
  size_t scan_lds = 0;
  const int rc = bank_geometry(pcen, window, stride, n_fft, hop, cols, &geo, &bank, &sa.nseg, &scan_lds);
  if (rc != HONK_OK) return rc;
  pcen::Params p;
  int power = 0;
  if (pcen) {
    const int prc = pcen::check_params(params, &p, &power);
    if (prc != HONK_OK) return prc;
  }
  TickPlan tp;
  const int trc = make_tick_plan(geo, bank, who, slots, n_slots, slot_ids, offsets, n_fed, window, stride,
                                 pcen && geo.mode == MODE_OVERLAP ? n_mels : 0, nullptr, nullptr, nullptr, 0, &tp);
  if (trc != HONK_OK) return trc;
  // the shape's own refusals (the mel-range table, the frame-tile kernel's LDS plan) come before the counts
  // are looked at: an empty tick -- no launch, no state touched -- tells a caller at construction whether any
  // later tick of the shape would be refused
  if (n_mels > MAX_MELS) return fail(HONK_ERR_UNSUPPORTED, "%s bank tick: more than %d mel bands", who, MAX_MELS);
  const int64_t nw = tp.p.windows;
  Args a;
  size_t lds = 0;
  {
    SegPlan sp;
    sp.p = honk_mfcc_segments_plan_t{};
    sp.p.windows = nw;
    sp.p.shared_frames = tp.shared_rows;
    sp.seg_tiles = tp.seg_tiles;
    // the log-mel and output tiles and the slots' destination tables reuse the span area
    const int tail_floats = pcen ? FT * (n_mels + 1) + 4 * FT : FT * (n_mels + 1) + FT * (n_dct + 1) + 5 * FT;
    const int lrc = segments_layout(geo, sp, who, window, stride, n_fft, hop, tail_floats, nullptr, n_fed, &a, &lds);
    if (lrc != HONK_OK) return lrc;
  }
  if (tp.p.samples_in == 0) return HONK_OK;  // (no new sample: no window, no tail moves)
  if (!chunks_dev || !table_dev || !state_dev || !workspace) return fail(HONK_ERR_ARG, "null pointer argument");
  if (nw > 0 && (!window_tbl || !mel_weights || (!pcen && !dct) || !out))
    return fail(HONK_ERR_ARG, "null pointer argument");
  if (workspace_bytes < (size_t)tp.p.workspace_bytes)
    return fail(HONK_ERR_WORKSPACE, "%s bank tick workspace: %zu bytes, %lld needed", who, workspace_bytes,
                (long long)tp.p.workspace_bytes);
  if (table_bytes < (size_t)tp.p.table_bytes)
    return fail(HONK_ERR_WORKSPACE, "%s bank tick table: %zu bytes, %lld needed", who, table_bytes,
                (long long)tp.p.table_bytes);
  if (state_bytes / (size_t)bank.p.slot_bytes < (size_t)n_slots)
    return fail(HONK_ERR_WORKSPACE, "%s bank tick state: %zu bytes, %lld slots of %lld needed", who, state_bytes,
                (long long)n_slots, (long long)bank.p.slot_bytes);
  BankGeo bg = bank.geo;
  bg.state = (char*)state_dev;
  const BankRec* table = (const BankRec*)table_dev;
  int16_t* pcm = (int16_t*)((char*)workspace + tp.pcm_offset);
  float* erows = (float*)((char*)workspace + 2 * MAX_MELS * sizeof(int));
  if (nw > 0) {
    a.pcm = pcm; a.window = window_tbl; a.melw = mel_weights; a.dct = pcen ? nullptr : dct;
    a.mrange = (const int*)workspace;
    a.out = pcen && geo.mode == MODE_OVERLAP ? erows : out;
    a.n_mels = n_mels; a.n_dct = pcen ? 0 : n_dct;
    a.btable = table;
    a.bank = bg;
  }
  const hipStream_t st = (hipStream_t)stream;
  const dim3 copy_grid((unsigned)n_fed, (unsigned)std::max<int64_t>(1, std::min<int64_t>(BANK_MAX_Y, cdiv(tp.max_len, 4 * BANK_THREADS))));
  hipLaunchKernelGGL(bank_assemble_kernel, copy_grid, dim3(BANK_THREADS), 0, st, table, bg, chunks_dev, pcm);
  HONK_LAUNCH_CHECK("bank_assemble_kernel");
  if (nw > 0) {
    hipLaunchKernelGGL(mel_range_kernel, dim3((unsigned)n_mels), dim3(64), 0, st, mel_weights, a.n_bins,
                       (int*)workspace);
    HONK_LAUNCH_CHECK("mel_range_kernel");
    const void* k1 = !pcen ? (const void*)mfcc_windows_kernel<EPI_MFCC, SRC_BANK>
                           : power == 1 ? (const void*)mfcc_windows_kernel<EPI_PCEN1, SRC_BANK>
                                        : (const void*)mfcc_windows_kernel<EPI_PCEN2, SRC_BANK>;
    if (lds > 64 * 1024)
      HONK_HIP_CHECK(hipFuncSetAttribute(k1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const dim3 grid((unsigned)tp.p.tiles), block(64 * WAVES);
    if (!pcen)
      hipLaunchKernelGGL((mfcc_windows_kernel<EPI_MFCC, SRC_BANK>), grid, block, lds, st, a);
    else if (power == 1)
      hipLaunchKernelGGL((mfcc_windows_kernel<EPI_PCEN1, SRC_BANK>), grid, block, lds, st, a);
    else
      hipLaunchKernelGGL((mfcc_windows_kernel<EPI_PCEN2, SRC_BANK>), grid, block, lds, st, a);
    HONK_LAUNCH_CHECK("mfcc_windows_kernel (bank tick)");
    if (pcen) {
      sa.e = erows; sa.out = out; sa.G = a.G; sa.table = nullptr; sa.n_rec = n_fed;
      sa.frames = a.frames; sa.n_mels = n_mels; sa.flo = geo.flo; sa.fhi = geo.fhi; sa.q = geo.q; sa.mode = geo.mode;
      if (geo.mode == MODE_OVERLAP) {
        sa.btable = table;
        sa.bank = bg;
      }
      if (scan_lds > 64 * 1024)
        HONK_HIP_CHECK(hipFuncSetAttribute((const void*)pcen_windows_scan_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      hipLaunchKernelGGL(pcen_windows_scan_kernel, dim3((unsigned)nw), dim3(SCAN_THREADS), scan_lds, st, sa, p);
      HONK_LAUNCH_CHECK("pcen_windows_scan_kernel");
    }
    if (bank.p.cache_rows > 0) {
      hipLaunchKernelGGL(bank_cache_kernel, dim3((unsigned)n_fed, (unsigned)cdiv(bank.p.cache_rows, FT)),
                         dim3(BANK_THREADS), 0, st, table, bg, pcen ? nullptr : out, cols, geo.p.frames, geo.flo,
                         geo.q);
      HONK_LAUNCH_CHECK("bank_cache_kernel");
    }
  }
  hipLaunchKernelGGL(bank_tail_kernel, copy_grid, dim3(BANK_THREADS), 0, st, table, bg, (const int16_t*)pcm);
  HONK_LAUNCH_CHECK("bank_tail_kernel");
  return HONK_OK;
}

}  // namespace mfccs
}  // namespace honk

using namespace honk;

extern "C" int honk_mfcc_windows_plan(int64_t samples, int32_t window, int32_t stride, int32_t n_fft, int32_t hop,
                                      int64_t first_window, int64_t n_windows, honk_mfcc_windows_plan_t* plan) {
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  mfccs::Plan pl;
  const int rc = mfccs::make_plan(samples, window, stride, n_fft, hop, first_window, n_windows, &pl);
  if (rc != HONK_OK) return rc;
  *plan = pl.p;
  return HONK_OK;
}

extern "C" int honk_mfcc_windows_i16(const int16_t* pcm_i16, int64_t samples, int32_t window, int32_t stride,
                                     int64_t first_window, int64_t n_windows, const float* window_tbl, int32_t n_fft,
                                     int32_t hop, const float* mel_weights, int32_t n_mels, const float* dct,
                                     int32_t n_dct, float* out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  using namespace mfccs;
  if (n_mels < 1 || n_dct < 1) return fail(HONK_ERR_ARG, "bad mfcc arguments");
  Plan pl;
  const int rc = make_plan(samples, window, stride, n_fft, hop, first_window, n_windows, &pl);
  if (rc != HONK_OK) return rc;
  if (n_windows == 0) return HONK_OK;
  if (!pcm_i16 || !window_tbl || !mel_weights || !dct || !out || !workspace)
    return fail(HONK_ERR_ARG, "null pointer argument");
  if (n_mels > MAX_MELS) return fail(HONK_ERR_UNSUPPORTED, "mfcc windows: more than %d mel bands", MAX_MELS);
  if (workspace_bytes < (size_t)pl.p.workspace_bytes)
    return fail(HONK_ERR_WORKSPACE, "mfcc windows workspace: %zu bytes, %lld needed", workspace_bytes,
                (long long)pl.p.workspace_bytes);
  Args a;
  a.pcm = pcm_i16; a.window = window_tbl; a.melw = mel_weights; a.dct = dct; a.mrange = (const int*)workspace;
  a.out = out;
  a.n_mels = n_mels; a.n_dct = n_dct;
  int64_t tiles;
  size_t lds;
  // the log-mel and output tiles and the slots' destination table reuse the span area
  const int lrc = layout(pl, "mfcc", window, stride, first_window, n_windows, n_fft, hop,
                         FT * (n_mels + 1) + FT * (n_dct + 1) + 3 * FT, &a, &tiles, &lds);
  if (lrc != HONK_OK) return lrc;
  hipLaunchKernelGGL(mel_range_kernel, dim3((unsigned)n_mels), dim3(64), 0, (hipStream_t)stream, mel_weights, a.n_bins,
                     (int*)workspace);
  HONK_LAUNCH_CHECK("mel_range_kernel");
  if (lds > 64 * 1024)  // (the plan's ceiling, so every shape and a captured call find it set)
    HONK_HIP_CHECK(hipFuncSetAttribute((const void*)mfcc_windows_kernel<EPI_MFCC>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL(mfcc_windows_kernel<EPI_MFCC>, dim3((unsigned)tiles), dim3(64 * WAVES), lds, (hipStream_t)stream,
                     a);
  HONK_LAUNCH_CHECK("mfcc_windows_kernel");
  return HONK_OK;
}

extern "C" int honk_pcen_windows_plan(int64_t samples, int32_t window, int32_t stride, int32_t n_fft, int32_t hop,
                                      int32_t n_mels, int64_t first_window, int64_t n_windows,
                                      honk_mfcc_windows_plan_t* plan) {
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  mfccs::Plan pl;
  int nseg;
  size_t scan_lds;
  const int rc = mfccs::make_pcen_plan(samples, window, stride, n_fft, hop, n_mels, first_window, n_windows, &pl,
                                       &nseg, &scan_lds);
  if (rc != HONK_OK) return rc;
  *plan = pl.p;
  return HONK_OK;
}

extern "C" int honk_pcen_windows_i16(const int16_t* pcm_i16, int64_t samples, int32_t window, int32_t stride,
                                     int64_t first_window, int64_t n_windows, const float* window_tbl, int32_t n_fft,
                                     int32_t hop, const float* mel_weights, int32_t n_mels,
                                     const honk_pcen_params_t* params, float* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  using namespace mfccs;
  Plan pl;
  ScanArgs sa;
  size_t scan_lds;
  const int rc = make_pcen_plan(samples, window, stride, n_fft, hop, n_mels, first_window, n_windows, &pl, &sa.nseg,
                                &scan_lds);
  if (rc != HONK_OK) return rc;
  pcen::Params p;
  int power;
  const int prc = pcen::check_params(params, &p, &power);
  if (prc != HONK_OK) return prc;
  if (n_windows == 0) return HONK_OK;
  if (!pcm_i16 || !window_tbl || !mel_weights || !out || !workspace)
    return fail(HONK_ERR_ARG, "null pointer argument");
  if (workspace_bytes < (size_t)pl.p.workspace_bytes)
    return fail(HONK_ERR_WORKSPACE, "pcen windows workspace: %zu bytes, %lld needed", workspace_bytes,
                (long long)pl.p.workspace_bytes);
  float* erows = (float*)((char*)workspace + 2 * MAX_MELS * sizeof(int));
  Args a;
  a.pcm = pcm_i16; a.window = window_tbl; a.melw = mel_weights; a.dct = nullptr; a.mrange = (const int*)workspace;
  a.out = pl.mode == MODE_OVERLAP ? erows : out;
  a.n_mels = n_mels; a.n_dct = 0;
  int64_t tiles;
  size_t lds;
  // the E tile and the slots' row table reuse the span area
  const int lrc = layout(pl, "pcen", window, stride, first_window, n_windows, n_fft, hop, FT * (n_mels + 1) + 2 * FT,
                         &a, &tiles, &lds);
  if (lrc != HONK_OK) return lrc;
  if (n_windows > 0x7fffffff) return fail(HONK_ERR_UNSUPPORTED, "pcen windows: too many windows in one call");
  sa.e = erows; sa.out = out; sa.G = a.G; sa.table = nullptr; sa.n_rec = 0;
  sa.frames = a.frames; sa.n_mels = n_mels; sa.flo = pl.flo; sa.fhi = pl.fhi; sa.q = pl.q; sa.mode = pl.mode;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mel_range_kernel, dim3((unsigned)n_mels), dim3(64), 0, st, mel_weights, a.n_bins,
                     (int*)workspace);
  HONK_LAUNCH_CHECK("mel_range_kernel");
  const void* k1 = power == 1 ? (const void*)mfcc_windows_kernel<EPI_PCEN1>
                              : (const void*)mfcc_windows_kernel<EPI_PCEN2>;
  if (lds > 64 * 1024)  // (the plan's ceiling, so every shape and a captured call find it set)
    HONK_HIP_CHECK(hipFuncSetAttribute(k1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (power == 1)
    hipLaunchKernelGGL(mfcc_windows_kernel<EPI_PCEN1>, dim3((unsigned)tiles), dim3(64 * WAVES), lds, st, a);
  else
    hipLaunchKernelGGL(mfcc_windows_kernel<EPI_PCEN2>, dim3((unsigned)tiles), dim3(64 * WAVES), lds, st, a);
  HONK_LAUNCH_CHECK("mfcc_windows_kernel (pcen energies)");
  if (scan_lds > 64 * 1024)
    HONK_HIP_CHECK(hipFuncSetAttribute((const void*)pcen_windows_scan_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL(pcen_windows_scan_kernel, dim3((unsigned)n_windows), dim3(SCAN_THREADS), scan_lds, st, sa, p);
  HONK_LAUNCH_CHECK("pcen_windows_scan_kernel");
  return HONK_OK;
}

extern "C" int honk_mfcc_segments_plan(const int64_t* offsets, int64_t n_rec, int32_t window, int32_t stride,
                                       int32_t n_fft, int32_t hop, int64_t* window0, void* table,
                                       size_t table_capacity, honk_mfcc_segments_plan_t* plan) {
  using namespace mfccs;
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  Plan geo;
  const int rc = make_plan(0, window, stride, n_fft, hop, 0, 0, &geo);
  if (rc != HONK_OK) return rc;
  SegPlan sp;
  const int src = make_segments_plan(geo, "mfcc", offsets, n_rec, false, 0, window, stride, 0, window0, (Rec*)table,
                                     table_capacity, &sp);
  if (src != HONK_OK) return src;
  *plan = sp.p;
  return HONK_OK;
}

extern "C" int honk_mfcc_segments_i16(const int16_t* pcm_i16, int64_t total_samples, const int64_t* offsets,
                                      int64_t n_rec, const void* table_dev, size_t table_bytes, int32_t window,
                                      int32_t stride, const float* window_tbl, int32_t n_fft, int32_t hop,
                                      const float* mel_weights, int32_t n_mels, const float* dct, int32_t n_dct,
                                      float* out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace mfccs;
  if (n_mels < 1 || n_dct < 1) return fail(HONK_ERR_ARG, "bad mfcc arguments");
  Plan geo;
  const int rc = make_plan(0, window, stride, n_fft, hop, 0, 0, &geo);
  if (rc != HONK_OK) return rc;
  SegPlan sp;
  const int src = make_segments_plan(geo, "mfcc", offsets, n_rec, true, total_samples, window, stride, 0, nullptr,
                                     nullptr, 0, &sp);
  if (src != HONK_OK) return src;
  if (sp.p.windows == 0) return HONK_OK;
  if (!pcm_i16 || !table_dev || !window_tbl || !mel_weights || !dct || !out || !workspace)
    return fail(HONK_ERR_ARG, "null pointer argument");
  if (n_mels > MAX_MELS) return fail(HONK_ERR_UNSUPPORTED, "mfcc segments: more than %d mel bands", MAX_MELS);
  if (workspace_bytes < (size_t)sp.p.workspace_bytes)
    return fail(HONK_ERR_WORKSPACE, "mfcc segments workspace: %zu bytes, %lld needed", workspace_bytes,
                (long long)sp.p.workspace_bytes);
  if (table_bytes < (size_t)sp.p.table_bytes)
    return fail(HONK_ERR_WORKSPACE, "mfcc segments table: %zu bytes, %lld needed", table_bytes,
                (long long)sp.p.table_bytes);
  Args a;
  a.pcm = pcm_i16; a.window = window_tbl; a.melw = mel_weights; a.dct = dct; a.mrange = (const int*)workspace;
  a.out = out;
  a.n_mels = n_mels; a.n_dct = n_dct;
  size_t lds;
  const int lrc = segments_layout(geo, sp, "mfcc", window, stride, n_fft, hop,
                                  FT * (n_mels + 1) + FT * (n_dct + 1) + 3 * FT, table_dev, n_rec, &a, &lds);
  if (lrc != HONK_OK) return lrc;
  hipLaunchKernelGGL(mel_range_kernel, dim3((unsigned)n_mels), dim3(64), 0, (hipStream_t)stream, mel_weights, a.n_bins,
                     (int*)workspace);
  HONK_LAUNCH_CHECK("mel_range_kernel");
  if (lds > 64 * 1024)
    HONK_HIP_CHECK(hipFuncSetAttribute((const void*)mfcc_windows_kernel<EPI_MFCC, SRC_SEG>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL((mfcc_windows_kernel<EPI_MFCC, SRC_SEG>), dim3((unsigned)sp.p.tiles), dim3(64 * WAVES), lds,
                     (hipStream_t)stream, a);
  HONK_LAUNCH_CHECK("mfcc_windows_kernel (segments)");
  return HONK_OK;
}

extern "C" int honk_pcen_segments_plan(const int64_t* offsets, int64_t n_rec, int32_t window, int32_t stride,
                                       int32_t n_fft, int32_t hop, int32_t n_mels, int64_t* window0, void* table,
                                       size_t table_capacity, honk_mfcc_segments_plan_t* plan) {
  using namespace mfccs;
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  Plan geo;
  int nseg;
  size_t scan_lds;
  const int rc = make_pcen_plan(0, window, stride, n_fft, hop, n_mels, 0, 0, &geo, &nseg, &scan_lds);
  if (rc != HONK_OK) return rc;
  SegPlan sp;
  const int src = make_segments_plan(geo, "pcen", offsets, n_rec, false, 0, window, stride,
                                     geo.mode == MODE_OVERLAP ? n_mels : 0, window0, (Rec*)table, table_capacity, &sp);
  if (src != HONK_OK) return src;
  *plan = sp.p;
  return HONK_OK;
}

extern "C" int honk_pcen_segments_i16(const int16_t* pcm_i16, int64_t total_samples, const int64_t* offsets,
                                      int64_t n_rec, const void* table_dev, size_t table_bytes, int32_t window,
                                      int32_t stride, const float* window_tbl, int32_t n_fft, int32_t hop,
                                      const float* mel_weights, int32_t n_mels, const honk_pcen_params_t* params,
                                      float* out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace mfccs;
  Plan geo;
  ScanArgs sa;
  size_t scan_lds;
  const int rc = make_pcen_plan(0, window, stride, n_fft, hop, n_mels, 0, 0, &geo, &sa.nseg, &scan_lds);
  if (rc != HONK_OK) return rc;
  pcen::Params p;
  int power;
  const int prc = pcen::check_params(params, &p, &power);
  if (prc != HONK_OK) return prc;
  SegPlan sp;
  const int src = make_segments_plan(geo, "pcen", offsets, n_rec, true, total_samples, window, stride,
                                     geo.mode == MODE_OVERLAP ? n_mels : 0, nullptr, nullptr, 0, &sp);
  if (src != HONK_OK) return src;
  if (sp.p.windows == 0) return HONK_OK;
  if (!pcm_i16 || !table_dev || !window_tbl || !mel_weights || !out || !workspace)
    return fail(HONK_ERR_ARG, "null pointer argument");
  if (workspace_bytes < (size_t)sp.p.workspace_bytes)
    return fail(HONK_ERR_WORKSPACE, "pcen segments workspace: %zu bytes, %lld needed", workspace_bytes,
                (long long)sp.p.workspace_bytes);
  if (table_bytes < (size_t)sp.p.table_bytes)
    return fail(HONK_ERR_WORKSPACE, "pcen segments table: %zu bytes, %lld needed", table_bytes,
                (long long)sp.p.table_bytes);
  float* erows = (float*)((char*)workspace + 2 * MAX_MELS * sizeof(int));
  Args a;
  a.pcm = pcm_i16; a.window = window_tbl; a.melw = mel_weights; a.dct = nullptr; a.mrange = (const int*)workspace;
  a.out = geo.mode == MODE_OVERLAP ? erows : out;
  a.n_mels = n_mels; a.n_dct = 0;
  size_t lds;
  const int lrc = segments_layout(geo, sp, "pcen", window, stride, n_fft, hop, FT * (n_mels + 1) + 2 * FT, table_dev,
                                  n_rec, &a, &lds);
  if (lrc != HONK_OK) return lrc;
  if (sp.p.windows > 0x7fffffff) return fail(HONK_ERR_UNSUPPORTED, "pcen segments: too many windows in one call");
  sa.e = erows; sa.out = out; sa.G = a.G; sa.table = (const Rec*)table_dev; sa.n_rec = n_rec;
  sa.frames = a.frames; sa.n_mels = n_mels; sa.flo = geo.flo; sa.fhi = geo.fhi; sa.q = geo.q; sa.mode = geo.mode;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mel_range_kernel, dim3((unsigned)n_mels), dim3(64), 0, st, mel_weights, a.n_bins,
                     (int*)workspace);
  HONK_LAUNCH_CHECK("mel_range_kernel");
  const void* k1 = power == 1 ? (const void*)mfcc_windows_kernel<EPI_PCEN1, SRC_SEG>
                              : (const void*)mfcc_windows_kernel<EPI_PCEN2, SRC_SEG>;
  if (lds > 64 * 1024)
    HONK_HIP_CHECK(hipFuncSetAttribute(k1, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (power == 1)
    hipLaunchKernelGGL((mfcc_windows_kernel<EPI_PCEN1, SRC_SEG>), dim3((unsigned)sp.p.tiles), dim3(64 * WAVES), lds, st, a);
  else
    hipLaunchKernelGGL((mfcc_windows_kernel<EPI_PCEN2, SRC_SEG>), dim3((unsigned)sp.p.tiles), dim3(64 * WAVES), lds, st, a);
  HONK_LAUNCH_CHECK("mfcc_windows_kernel (segments, pcen energies)");
  if (scan_lds > 64 * 1024)
    HONK_HIP_CHECK(hipFuncSetAttribute((const void*)pcen_windows_scan_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL(pcen_windows_scan_kernel, dim3((unsigned)sp.p.windows), dim3(SCAN_THREADS), scan_lds, st, sa, p);
  HONK_LAUNCH_CHECK("pcen_windows_scan_kernel");
  return HONK_OK;
}

extern "C" int honk_stream_bank_plan(int32_t window, int32_t stride, int32_t n_fft, int32_t hop, int32_t row_floats,
                                     honk_stream_bank_plan_t* plan) {
  using namespace mfccs;
  if (!plan) return fail(HONK_ERR_ARG, "null pointer argument");
  if (row_floats < 1) return fail(HONK_ERR_ARG, "stream bank: row_floats < 1");
  Plan geo;
  const int rc = make_plan(0, window, stride, n_fft, hop, 0, 0, &geo);
  if (rc != HONK_OK) return rc;
  Args a;
  int64_t tiles;
  size_t lds;
  const int lrc = layout(geo, "stream bank", window, stride, 0, 0, n_fft, hop, 0, &a, &tiles, &lds);
  if (lrc != HONK_OK) return lrc;
  BankPlan bank;
  make_bank_plan(geo, window, row_floats, &bank);
  *plan = bank.p;
  return HONK_OK;
}

extern "C" int honk_mfcc_bank_tick_plan(const honk_bank_slot_t* slots, int64_t n_slots, const int64_t* slot_ids,
                                        const int64_t* chunk_offsets, int64_t n_fed, int32_t window, int32_t stride,
                                        int32_t n_fft, int32_t hop, int32_t n_dct, int64_t* window0,
                                        honk_bank_slot_t* next, void* table, size_t table_capacity,
                                        honk_bank_tick_plan_t* plan) {
  return mfccs::bank_tick_plan(false, slots, n_slots, slot_ids, chunk_offsets, n_fed, window, stride, n_fft, hop, n_dct,
                               window0, next, table, table_capacity, plan);
}

extern "C" int honk_pcen_bank_tick_plan(const honk_bank_slot_t* slots, int64_t n_slots, const int64_t* slot_ids,
                                        const int64_t* chunk_offsets, int64_t n_fed, int32_t window, int32_t stride,
                                        int32_t n_fft, int32_t hop, int32_t n_mels, int64_t* window0,
                                        honk_bank_slot_t* next, void* table, size_t table_capacity,
                                        honk_bank_tick_plan_t* plan) {
  return mfccs::bank_tick_plan(true, slots, n_slots, slot_ids, chunk_offsets, n_fed, window, stride, n_fft, hop, n_mels,
                               window0, next, table, table_capacity, plan);
}

extern "C" int honk_mfcc_bank_tick_i16(const int16_t* chunks_dev, const honk_bank_slot_t* slots, int64_t n_slots,
                                       const int64_t* slot_ids, const int64_t* chunk_offsets, int64_t n_fed,
                                       const void* table_dev, size_t table_bytes, void* state_dev, size_t state_bytes,
                                       int32_t window, int32_t stride, const float* window_tbl, int32_t n_fft,
                                       int32_t hop, const float* mel_weights, int32_t n_mels, const float* dct,
                                       int32_t n_dct, float* out, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  return mfccs::bank_tick(nullptr, false, chunks_dev, slots, n_slots, slot_ids, chunk_offsets, n_fed, table_dev,
                          table_bytes, state_dev, state_bytes, window, stride, window_tbl, n_fft, hop, mel_weights,
                          n_mels, dct, n_dct, out, workspace, workspace_bytes, stream);
}

extern "C" int honk_pcen_bank_tick_i16(const int16_t* chunks_dev, const honk_bank_slot_t* slots, int64_t n_slots,
                                       const int64_t* slot_ids, const int64_t* chunk_offsets, int64_t n_fed,
                                       const void* table_dev, size_t table_bytes, void* state_dev, size_t state_bytes,
                                       int32_t window, int32_t stride, const float* window_tbl, int32_t n_fft,
                                       int32_t hop, const float* mel_weights, int32_t n_mels,
                                       const honk_pcen_params_t* params, float* out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return mfccs::bank_tick(params, true, chunks_dev, slots, n_slots, slot_ids, chunk_offsets, n_fed, table_dev,
                          table_bytes, state_dev, state_bytes, window, stride, window_tbl, n_fft, hop, mel_weights,
                          n_mels, nullptr, 0, out, workspace, workspace_bytes, stream);
}
