// SpeechModel forward (cnn-trad-pool2, cnn-one-*, cnn-tpool*, cnn-tstride*) for
// gfx950, fp32.  Reference: /root/reference/utils/model.py:123-205.
//
//   conv1 (+bias, ReLU) -> maxpool1 -> [conv2 (+bias, ReLU) -> maxpool2]
//   -> flatten (c,h,w) -> [lin] -> [dnn1 (+ReLU unless tf_variant)] -> [dnn2]
//   -> output                                  (dropout = identity in eval)
//
// Every conv and every Linear is one implicit GEMM on fp32 MFMA
// (v_mfma_f32_16x16x4_f32), computed transposed so stores are coalesced:
//     D[n][m] = bias[n] + sum_k W[n][k] * X[k][m]
// n = out channel, m = (clip, oh, ow) output pixel, k = (ci, kh, kw) -- the
// OIHW weight tensor IS the [N][K] operand, X is gathered on the fly from the
// NCHW input (valid convolution, stride (sh, sw)).  A Linear is the same GEMM
// with H = W = KH = KW = 1.  Activations stay NCHW so flatten is free.
#include "common.h"

namespace honk {
namespace cnn {

constexpr int BM = 128;  // output pixels per block
constexpr int BN = 64;   // output channels per block
constexpr int BK = 32;   // reduction slice per LDS stage
constexpr int PADM = 4;  // LDS row padding (floats)
constexpr int KTAB = 4096;  // max K with an LDS k->offset table (else computed)

struct GemmArgs {
  const float* in;   // NCHW [B][Cin][H][W]
  const float* w;    // [N][K]
  const float* bias; // [N] or nullptr
  float* out;        // NCHW [B][N][OH][OW], or [B][N][OH/2][OW/2] when pool2 fused
  int64_t M;         // GEMM rows: B*OH*OW, or B*PH*PW*4 (pool2: 4 window members per pooled pixel)
  int N, K;
  int Cin, H, W, KH, KW, SH, SW, OH, OW;
  int DH, DW;        // dilation (1: the SpeechModel convs; the res block convs of honk_conv_same_f32)
  int PH, PW;        // pooled output dims (pool2 fused)
  int relu;
  int nhwc_x3;       // POOL2 only: 1 = store [B][PH][PW][hi N | lo N] bf16 (conv2x3_kernel's input),
                     // 2 = [B][PH][PW][N] fp32 (conv2f_kernel's input), instead of NCHW fp32
};

// D[n][m] = act(bias[n] + sum_k W[n][k] * X[k][m]) on v_mfma_f32_16x16x4_f32.
// 256 threads = 4 waves; wave w owns pixels [32w, 32w+32) of the block's 128
// (2 m-tiles) and all 64 out channels (4 n-tiles) -> 8 accumulators.  X is
// gathered from NCHW through a per-block k->offset table in LDS (no integer
// division in the K loop); W rows are read 16 B at a time.  Slices are staged
// LDS <- registers with the next slice's global loads in flight during the MFMAs.
// POOL2: rows are ordered (clip, ph, pw, 2x2 member) so the four members of a
// max-pool window sit in 4 adjacent lanes: the epilogue max-reduces them with
// two lane swaps and stores only the pooled value (nn.MaxPool2d((2,2)) fused).
//
// X3 (bf16x3 mode): the same GEMM with every operand split at staging time into
// bf16 (hi, lo) = (bf16(v), bf16(v - hi)), stored k-contiguous ([m][k], [n][k])
// so a lane's 8 consecutive k are one 16-byte MFMA fragment, and each 32-deep
// slice is ONE v_mfma_f32_16x16x32_bf16 step of 3 products (hi*hi + hi*lo +
// lo*hi) per tile pair, fp32 accumulation -- the fp32 1e-4 bar at bf16 MFMA rates.
typedef __bf16 cbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4c __attribute__((ext_vector_type(4)));
constexpr int BKP = BK + 8;  // X3 LDS row pitch (bf16): 80 B keeps 16-lane fragment reads conflict-free

// max / relu with torch's NaN behaviour (a NaN propagates)
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float relu_nan(float v) { return v <= 0.f ? 0.f : v; }

template <bool POOL2, bool X3>
__global__ __launch_bounds__(256) void conv_gemm_kernel(GemmArgs a) {
  // fp32: Ws[2][BK][BN + PADM], Xs[2][BK][BM + PADM] (floats)
  // X3:   Wh[2 buf][2 part][BN][BKP], Xh[2 buf][2 part][BM][BKP] (bf16)
  constexpr int WS_BYTES = X3 ? 2 * 2 * BN * BKP * 2 : 2 * BK * (BN + PADM) * 4;
  constexpr int XS_BYTES = X3 ? 2 * 2 * BM * BKP * 2 : 2 * BK * (BM + PADM) * 4;
  __shared__ __attribute__((aligned(16))) char wsm[WS_BYTES];
  __shared__ __attribute__((aligned(16))) char xsm[XS_BYTES];
  float (*Ws)[BK][BN + PADM] = (float (*)[BK][BN + PADM])wsm;
  float (*Xs)[BK][BM + PADM] = (float (*)[BK][BM + PADM])xsm;
  __bf16 (*Wh)[2][BN][BKP] = (__bf16 (*)[2][BN][BKP])wsm;
  __bf16 (*Xh)[2][BM][BKP] = (__bf16 (*)[2][BM][BKP])xsm;
  __shared__ int ktab[KTAB];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int KHW = a.KH * a.KW;
  const bool use_tab = a.K <= KTAB;
  if (use_tab)
    for (int k = tid; k < a.K; k += 256) {
      const int ci = k / KHW, rem = k - ci * KHW;
      const int kh = rem / a.KW, kw = rem - kh * a.KW;
      ktab[k] = (ci * a.H + kh * a.DH) * a.W + kw * a.DW;
    }

  // X staging: thread owns pixel column mm = tid % 128 and rows kk = tid/128 + 2r
  // (X3: the 16 consecutive rows 16 (tid/128) + r)
  const int mm = tid & (BM - 1);
  const int kq = tid >> 7;
  const int64_t mglob = m0 + mm;
  const bool mvalid = mglob < a.M;
  int64_t xbase = 0;
  if (mvalid) {
    int oh, ow;
    int64_t b;
    if (POOL2) {
      const int64_t q = mglob >> 2;
      const int sub = (int)(mglob & 3);
      const int PHW = a.PH * a.PW;
      b = q / PHW;
      const int pp = (int)(q - b * PHW);
      const int ph = pp / a.PW, pw = pp - ph * a.PW;
      oh = 2 * ph + (sub >> 1);
      ow = 2 * pw + (sub & 1);
    } else {
      const int OHW = a.OH * a.OW;
      b = mglob / OHW;
      const int pix = (int)(mglob - b * OHW);
      oh = pix / a.OW;
      ow = pix - oh * a.OW;
    }
    xbase = b * ((int64_t)a.Cin * a.H * a.W) + (int64_t)(oh * a.SH) * a.W + ow * a.SW;
  }
  // W staging: thread owns row n = tid/4, columns (tid%4)*8 .. +7
  const int wn_row = tid >> 2;
  const int wk0 = (tid & 3) * 8;
  const bool wvec = (a.K & 3) == 0 && ((((uintptr_t)a.w) & 15) == 0);

  float xr[16], wv[8];
  auto koffset = [&](int k) -> int {
    if (use_tab) return ktab[k];
    const int ci = k / KHW, rem = k - ci * KHW;
    const int kh = rem / a.KW, kw = rem - kh * a.KW;
    return (ci * a.H + kh * a.DH) * a.W + kw * a.DW;
  };
  auto load_slice = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + (X3 ? kq * 16 + r : kq + 2 * r);
      xr[r] = (mvalid && k < a.K) ? a.in[xbase + koffset(k)] : 0.f;
    }
    const int n = n0 + wn_row;
    const int kb = k0 + wk0;
    if (n < a.N && wvec && kb + 8 <= a.K) {
      const f32x4 u = *(const f32x4*)(a.w + (int64_t)n * a.K + kb);
      const f32x4 v = *(const f32x4*)(a.w + (int64_t)n * a.K + kb + 4);
      wv[0] = u[0]; wv[1] = u[1]; wv[2] = u[2]; wv[3] = u[3];
      wv[4] = v[0]; wv[5] = v[1]; wv[6] = v[2]; wv[7] = v[3];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) wv[j] = (n < a.N && kb + j < a.K) ? a.w[(int64_t)n * a.K + kb + j] : 0.f;
    }
  };
  auto store_slice = [&](int buf) {
    if constexpr (X3) {
      cbf16x8 xh[2], xl[2], whv, wlv;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const __bf16 h = (__bf16)xr[r];
        xh[r >> 3][r & 7] = h;
        xl[r >> 3][r & 7] = (__bf16)(xr[r] - (float)h);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)wv[j];
        whv[j] = h;
        wlv[j] = (__bf16)(wv[j] - (float)h);
      }
      *(cbf16x8*)&Xh[buf][0][mm][kq * 16] = xh[0];
      *(cbf16x8*)&Xh[buf][0][mm][kq * 16 + 8] = xh[1];
      *(cbf16x8*)&Xh[buf][1][mm][kq * 16] = xl[0];
      *(cbf16x8*)&Xh[buf][1][mm][kq * 16 + 8] = xl[1];
      *(cbf16x8*)&Wh[buf][0][wn_row][wk0] = whv;
      *(cbf16x8*)&Wh[buf][1][wn_row][wk0] = wlv;
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) Xs[buf][kq + 2 * r][mm] = xr[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) Ws[buf][wk0 + j][wn_row] = wv[j];
    }
  };

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  __syncthreads();  // ktab ready
  const int nslices = (a.K + BK - 1) / BK;
  load_slice(0);
  store_slice(0);
  __syncthreads();
  for (int t = 0; t < nslices; ++t) {
    const int buf = t & 1;
    if (t + 1 < nslices) load_slice((t + 1) * BK);
    if constexpr (X3) {
      // one 32-deep k-step: lane (g, i16) holds k = 8g .. 8g+7 of row i16
      const int kc = (lane >> 4) * 8, r16 = lane & 15;
      cbf16x8 aw[2][4], bx[2][2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) aw[pt][i] = *(const cbf16x8*)&Wh[buf][pt][i * 16 + r16][kc];
#pragma unroll
        for (int j = 0; j < 2; ++j) bx[pt][j] = *(const cbf16x8*)&Xh[buf][pt][wave * 32 + j * 16 + r16][kc];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0][i], bx[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0][i], bx[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[1][i], bx[0][j], acc[i][j], 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int ks = 0; ks < BK / 4; ++ks) {
        const int kk = ks * 4 + (lane >> 4);
        float av[4], bv[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = Ws[buf][kk][i * 16 + (lane & 15)];
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = Xs[buf][kk][wave * 32 + j * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
      }
    }
    if (t + 1 < nslices) store_slice(buf ^ 1);
    __syncthreads();
  }

  // epilogue: D[n][m]; lane holds rows n = (lane>>4)*4 + r, column m = lane & 15
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t m = m0 + wave * 32 + j * 16 + (lane & 15);
    const bool mok = m < a.M;
    int64_t obase;
    int64_t plane;
    if (POOL2) {
      const int64_t q = m >> 2;
      const int PHW = a.PH * a.PW;
      const int64_t b = q / PHW;
      obase = b * (int64_t)a.N * PHW + (q - b * PHW);
      plane = PHW;
    } else {
      const int OHW = a.OH * a.OW;
      const int64_t b = m / OHW;
      obase = b * (int64_t)a.N * OHW + (m - b * OHW);
      plane = OHW;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float pooled[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + i * 16 + (lane >> 4) * 4 + r;
        float v = acc[i][j][r] + ((a.bias && n < a.N) ? a.bias[n] : 0.f);
        if (a.relu) v = v <= 0.f ? 0.f : v;  // NaN passes, as torch.relu
        if (POOL2) {  // max over the 2x2 window = lanes l, l^1, l^2, l^3 (same n); NaN propagates
          v = nanmax(v, __shfl_xor(v, 1));
          v = nanmax(v, __shfl_xor(v, 2));
          if (a.nhwc_x3) pooled[r] = v;
          else if ((lane & 3) == 0 && mok && n < a.N) a.out[obase + (int64_t)n * plane] = v;
        } else if (mok && n < a.N) {
          a.out[obase + (int64_t)n * plane] = v;
        }
      }
      if (POOL2 && a.nhwc_x3 == 2 && (lane & 3) == 0 && mok) {
        // the lane's 4 consecutive channels of its pooled pixel: one 16-B NHWC store
        const int n = n0 + i * 16 + (lane >> 4) * 4;
        if (n + 3 < a.N)
          *(f32x4*)(a.out + (m >> 2) * (int64_t)a.N + n) = f32x4{pooled[0], pooled[1], pooled[2], pooled[3]};
      }
      if (POOL2 && a.nhwc_x3 == 1 && (lane & 3) == 0 && mok) {
        // the lane's 4 consecutive channels of its pooled pixel, split into bf16
        // (hi, lo) runs of the [hi N | lo N] pixel (N == 64: host-checked)
        const int n = n0 + i * 16 + (lane >> 4) * 4;
        bf16x4c hv, lv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          hv[r] = (__bf16)pooled[r];
          lv[r] = (__bf16)(pooled[r] - (float)hv[r]);
        }
        __bf16* px = (__bf16*)a.out + (m >> 2) * (int64_t)(2 * a.N);
        *(bf16x4c*)(px + n) = hv;
        *(bf16x4c*)(px + a.N + n) = lv;
      }
    }
  }
}

__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      int64_t planes, int H, int W, int KH, int KW) {
  const int PH = H / KH, PW = W / KW;
  const int64_t total = planes * PH * PW;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int pw = (int)(i % PW);
  const int64_t t = i / PW;
  const int ph = (int)(t % PH);
  const int64_t pl = t / PH;
  const float* p = in + pl * H * W + (int64_t)(ph * KH) * W + pw * KW;
  float m = p[0];
  for (int a = 0; a < KH; ++a)
    for (int b = 0; b < KW; ++b) {
      const float v = p[a * W + b];
      m = (v > m || v != v) ? v : m;  // NaN propagates like torch
    }
  out[i] = m;
}


// ---------------------------------------------------------------------------- //
// conv2 of cnn-trad-pool2 (64 -> <= 64 channels, stride 1, no pool after it) in
// bf16x3 on an NHWC hi/lo input: the whole clip is one tile.
//
// The input (conv1 + ReLU + MaxPool2d(2,2) output, written by conv_gemm_kernel's
// nhwc_x3 epilogue as [B][PH][PW][hi 64 | lo 64] bf16) is staged per clip in two
// 32-channel halves: one LDS image of PH*PW pixels x 128 B ([hi 32 | lo 32]) per
// half, filled by LDS-DMA, its 16-B chunks XOR-swizzled by pixel (chunk c of
// pixel P at slot P*8 + (c ^ (P & 7))) so a fragment read spreads over the banks.
// Implicit GEMM, weights as the MFMA A operand (16 out channels x 32 k), the
// image as B (32 k x 16 output pixels): k-step s = (half, tap kh*KW + kw) over
// the half's 32 channels, lane group g holding channels 8g .. 8g+7.
// 4 waves (one per SIMD): wave = (n-group: out tiles 2ng, 2ng+1) x (m-group: MT
// consecutive 16-pixel tiles of the clip's OH*OW outputs).  Each k-step reads
// the wave's MT A fragment pairs from LDS and its 4 weight fragments (hi, lo of
// 2 out tiles, pre-split by pack_conv2x3_kernel, L2-resident) from global, both
// one k-step ahead, and runs 6 MT MFMAs (hi*hi + hi*lo + lo*hi).
// Epilogue: bias + ReLU, NCHW fp32 stores (flatten order of model.py:194).
// ---------------------------------------------------------------------------- //
constexpr int C2X3_IMG = 96 * 1024;  // LDS bytes of one half image (PH*PW*128 <= this)
// (ablations, round 1: no image DMA -10 %, no A-fragment reads -9 %, L1-resident
// weights -5 %, all three -26 %)

struct Conv2X3Args {
  const __bf16* in;    // [B][PH][PW][hi 64 | lo 64]
  const uint4* wfrag;  // [2*ntap k-steps][4 out tiles][2 parts][64 lanes] x 16 B
  const float* bias;   // [N]
  float* out;          // [B][N][OH][OW]
  int B, PH, PW, KW, ntap, OH, OW, N;
};

template <int MT>
__global__ __launch_bounds__(256, 1) void conv2x3_kernel(Conv2X3Args a) {
  __shared__ __attribute__((aligned(16))) char img[C2X3_IMG];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave & 1, mg = wave >> 1;
  const int g = lane >> 4, i16 = lane & 15;
  const int npx = a.PH * a.PW;
  const int ohw = a.OH * a.OW;
  const int chunks = npx * 8;
  const int pieces = (chunks + 63) / 64;
  const int clip_bytes = npx * 256;

  // per m-tile: the lane's output pixel -> its input pixel at tap (0, 0)
  int P0[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int p = (mg * MT + m) * 16 + i16;
    const int oh = p / a.OW, ow = p - oh * a.OW;
    P0[m] = p < ohw ? oh * a.PW + ow : 0;
  }
  const uint4* wl = a.wfrag + ng * 2 * 2 * 64 + lane;  // (s, nt = 2 ng + j, part) -> wl[(s*4 + j)*... ]

  typedef uint4 AFr[MT][2];
  typedef uint4 WFr[2][2];
  auto loadA = [&](AFr& A, int delta) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int P = P0[m] + delta;
      const int ad = ((P << 3) + (g ^ (P & 7))) << 4;
      A[m][0] = *(const uint4*)(img + ad);
      A[m][1] = *(const uint4*)(img + (ad ^ 64));
    }
  };
  auto loadW = [&](WFr& Wr, int s) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) Wr[j][pt] = wl[((s * 4 + j) * 2 + pt) * 64];
  };
  f32x4 acc[MT][2];
  auto mma = [&](const AFr& A, const WFr& Wr) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cbf16x8, Wr[j][t == 2 ? 1 : 0]),
                                                              __builtin_bit_cast(cbf16x8, A[m][t == 1 ? 1 : 0]),
                                                              acc[m][j], 0, 0, 0);
  };
  auto delta = [&](int t) {
    const int kh = t / a.KW;
    return kh * a.PW + (t - kh * a.KW);
  };

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.in + (size_t)b * clip_bytes), (short)0, clip_bytes, 0x00020000);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < 2; ++h) {
      __syncthreads();  // every wave is done reading the previous image
      for (int pc = wave; pc < pieces; pc += 4) {
        const int st = __builtin_amdgcn_readfirstlane(min(pc * 64, chunks - 64));
        const int L = st + lane;
        const int P = L >> 3, c = (L & 7) ^ (P & 7);
        const unsigned voff = (unsigned)(P * 256 + (c >> 2) * 128 + h * 64 + (c & 3) * 16);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + st * 16), 16,
                                                 voff, 0, 0, 0);
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's pieces landed
      __syncthreads();                     // ... and every wave's
      const int s0 = h * a.ntap;
      AFr A0, A1;
      WFr W0, W1;
      loadW(W0, s0);
      loadA(A0, 0);
      for (int t = 0; t < a.ntap; t += 2) {  // ntap even (host-checked)
        loadW(W1, s0 + t + 1);
        loadA(A1, delta(t + 1));
        mma(A0, W0);
        if (t + 2 < a.ntap) {
          loadW(W0, s0 + t + 2);
          loadA(A0, delta(t + 2));
        }
        mma(A1, W1);
      }
    }
    // epilogue: lane (g, i16) holds out channels (2 ng + j) 16 + 4 g + r of pixel p
    float* ob = a.out + (size_t)b * a.N * ohw;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int p = (mg * MT + m) * 16 + i16;
      if (p < ohw) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = (2 * ng + j) * 16 + 4 * g + r;
            if (n < a.N) ob[(size_t)n * ohw + p] = relu_nan(acc[m][j][r] + a.bias[n]);
          }
      }
    }
  }
}

// conv2 weights [N][64][KH][KW] fp32 -> conv2x3_kernel's fragments: k-step
// s = half * ntap + tap, out tile nt, part (hi, lo), lane (g, i16):
// 8 bf16 of W[16 nt + i16][32 half + 8 g + j][tap] (zero past N)
__global__ void pack_conv2x3_kernel(const float* __restrict__ w, __bf16* __restrict__ frag, int N, int ntap) {
  const int total = 2 * ntap * 4 * 2 * 64 * 8;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int r = i;
  const int j = r & 7; r >>= 3;
  const int lane = r & 63; r >>= 6;
  const int pt = r & 1; r >>= 1;
  const int nt = r & 3; r >>= 2;
  const int s = r;
  const int h = s / ntap, t = s - h * ntap;
  const int co = nt * 16 + (lane & 15);
  const int ci = 32 * h + 8 * (lane >> 4) + j;
  const float v = co < N ? w[((size_t)co * 64 + ci) * ntap + t] : 0.f;
  const __bf16 hi = (__bf16)v;
  frag[i] = pt == 0 ? hi : (__bf16)(v - (float)hi);
}


// ---------------------------------------------------------------------------- //
// The same conv2 in fp32 (HONK_PREC_F32, config C2 as BASELINE.json names it) on
// v_mfma_f32_16x16x4_f32: the conv2x3_kernel design -- the whole clip one tile, two
// 32-channel half images by LDS-DMA (fp32 NHWC input from conv_gemm_kernel's
// nhwc_x3 = 2 epilogue: the half image is 128 B per pixel, the bf16 hi/lo one's
// size), 16-B chunks XOR-swizzled by pixel, 4 waves = 2 out-tile pairs x 2 groups
// of MT m-tiles, accumulators for the whole clip in VGPRs.
//   k-chunk (tap t, q): lane group g reads chunk 4q + g of its pixel (channels
//   32h + 16q + 4g .. +3 as one 16-B read); MFMA e = 0..3 takes element e, so one
//   read feeds 4 MFMAs per out tile; the weight A operand of MFMA e is
//   W[co][32h + 16q + 4g + e][t], pre-packed per lane as one float4 per chunk and
//   out tile (pack_conv2f_kernel, L2-resident), loaded one chunk ahead with the
//   activations.  fp32 products and accumulation: the fmaf chain of the reference
//   conv in another order (1e-4 parity).
// ---------------------------------------------------------------------------- //
struct Conv2FArgs {
  const float* in;      // [B][PH][PW][64] fp32
  const f32x4* wfrag;   // [2 h][ntap][2 q][4 out tiles][64 lanes]
  const float* bias;    // [N]
  float* out;           // [B][N][OH][OW]
  int B, PH, PW, KW, ntap, OH, OW, N;
};

template <int MT>
__global__ __launch_bounds__(256, 1) void conv2f_kernel(Conv2FArgs a) {
  __shared__ __attribute__((aligned(16))) char img[C2X3_IMG];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave & 1, mg = wave >> 1;
  const int g = lane >> 4, i16 = lane & 15;
  const int npx = a.PH * a.PW;
  const int ohw = a.OH * a.OW;
  const int chunks = npx * 8;
  const int pieces = (chunks + 63) / 64;
  const int clip_bytes = npx * 256;

  int P0[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int p = (mg * MT + m) * 16 + i16;
    const int oh = p / a.OW, ow = p - oh * a.OW;
    P0[m] = p < ohw ? oh * a.PW + ow : 0;
  }
  const f32x4* wl = a.wfrag + ng * 2 * 64 + lane;

  typedef f32x4 BFr[MT];
  typedef f32x4 WFr[2];
  auto loadB = [&](BFr& Bv, int delta, int q) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int P = P0[m] + delta;
      Bv[m] = *(const f32x4*)(img + (((P << 3) + ((4 * q + g) ^ (P & 7))) << 4));
    }
  };
  auto loadW = [&](WFr& Wv, int c) {  // c = (h * ntap + t) * 2 + q
#pragma unroll
    for (int j = 0; j < 2; ++j) Wv[j] = wl[(c * 4 + j) * 64];
  };
  f32x4 acc[MT][2];
  auto mma = [&](const BFr& Bv, const WFr& Wv) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Wv[j][e], Bv[m][e], acc[m][j], 0, 0, 0);
  };
  auto delta = [&](int t) {
    const int kh = t / a.KW;
    return kh * a.PW + (t - kh * a.KW);
  };

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.in + (size_t)b * clip_bytes), (short)0, clip_bytes, 0x00020000);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < 2; ++h) {
      __syncthreads();  // every wave is done reading the previous image
      for (int pc = wave; pc < pieces; pc += 4) {
        const int st = __builtin_amdgcn_readfirstlane(min(pc * 64, chunks - 64));
        const int L = st + lane;
        const int P = L >> 3, c = (L & 7) ^ (P & 7);
        const unsigned voff = (unsigned)(P * 256 + h * 128 + c * 16);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + st * 16), 16,
                                                 voff, 0, 0, 0);
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's pieces landed
      __syncthreads();                     // ... and every wave's
      const int nch = 2 * a.ntap;          // chunks of this half: (tap, q)
      const int c0 = h * nch;
      BFr B0, B1;
      WFr W0, W1;
      loadW(W0, c0);
      loadB(B0, 0, 0);
      for (int c = 0; c < nch; c += 2) {  // chunk c: tap c / 2, q = 0; c + 1: q = 1
        const int dt = delta(c >> 1);
        loadW(W1, c0 + c + 1);
        loadB(B1, dt, 1);
        mma(B0, W0);
        if (c + 2 < nch) {
          loadW(W0, c0 + c + 2);
          loadB(B0, delta((c >> 1) + 1), 0);
        }
        mma(B1, W1);
      }
    }
    float* ob = a.out + (size_t)b * a.N * ohw;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int p = (mg * MT + m) * 16 + i16;
      if (p < ohw) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = (2 * ng + j) * 16 + 4 * g + r;
            if (n < a.N) ob[(size_t)n * ohw + p] = relu_nan(acc[m][j][r] + a.bias[n]);
          }
      }
    }
  }
}

// conv2 weights [N][64][KH][KW] fp32 -> conv2f_kernel's fragments: chunk
// c = (h * ntap + t) * 2 + q, out tile nt, lane (g, i16): the float4
// W[16 nt + i16][32 h + 16 q + 4 g + e][t], e = 0..3 (zero past N)
__global__ void pack_conv2f_kernel(const float* __restrict__ w, float* __restrict__ frag, int N, int ntap) {
  const int total = 2 * ntap * 2 * 4 * 64 * 4;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int r = i;
  const int e = r & 3; r >>= 2;
  const int lane = r & 63; r >>= 6;
  const int nt = r & 3; r >>= 2;
  const int c = r;  // (h * ntap + t) * 2 + q
  const int q = c & 1, ht = c >> 1;
  const int h = ht / ntap, t = ht - h * ntap;
  const int co = nt * 16 + (lane & 15);
  const int ci = 32 * h + 16 * q + 4 * (lane >> 4) + e;
  frag[i] = co < N ? w[((size_t)co * 64 + ci) * ntap + t] : 0.f;
}

// ---------------------------------------------------------------------------- //
// conv1 + ReLU + MaxPool2d(2,2) of cnn-trad-pool2 (1 -> 64 channels, 20 x 8
// filter, stride 1) in bf16x3, writing conv2x3_kernel's NHWC hi/lo input.
// One clip per tile, 8 waves = 2 n-groups (out tiles 2ng, 2ng+1) x 4 m-groups.
//   K = 160 = 5 k-steps: lane group g of k-step s holds kh = 4s + g, kw = 0..7,
//   i.e. 8 consecutive input pixels of one row.  The clip is staged in LDS as a
//   "shifted-row" image: entry (r, c) = x[r][c .. c+7] as 8 bf16, hi and lo in
//   separate planes, c = 0 .. 31 (the pooled output's columns), entry slot
//   r*32 + ((c + 8 r) & 31) (16-B entries: conflict-free fragment reads), so an
//   A fragment is ONE aligned 16-B read and k-step s adds a fixed 2 KiB offset.
//   Weights: the wave's 2 out tiles x 5 k-steps x (hi, lo) fragments live in
//   VGPRs for the whole launch (W[co][kh][0..7] is 8 contiguous floats).
//   M = pooled members (ph, pw, 2x2 member) so the 4 members of a window sit in
//   lanes l .. l^3 of one MFMA column group: bias, ReLU, 2 lane-swap maxes, then
//   the lane with member 0 stores 4 channels' hi and lo runs (8 B each).
// ---------------------------------------------------------------------------- //
constexpr int C1X3_KH = 20, C1X3_KW = 8, C1X3_COLS = 32, C1X3_HMAX = 101;
// (prefetching the next clip's rows during this clip's MFMAs measured 0.4 % slower:
// 15 VGPR spills)
constexpr int C1X3_PLANE = C1X3_HMAX * C1X3_COLS * 16;  // bytes of one (hi or lo) plane

struct Conv1X3Args {
  const float* x;     // [B][H][W]
  const float* w;     // [64][1][20][8]
  const float* bias;  // [64]
  __bf16* out;        // [B][PH][PW][hi 64 | lo 64]
  int B, H, W, PH, PW;
};

__global__ __launch_bounds__(512, 1) void conv1x3_kernel(Conv1X3Args a) {
  __shared__ __attribute__((aligned(16))) char img[2 * C1X3_PLANE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave & 1, mg = wave >> 1;
  const int g = lane >> 4, i16 = lane & 15;
  const int nmt = a.PH * a.PW / 4;  // 16-row m-tiles of pooled members (PH*PW % 4 == 0: host-checked)
  const int clip_floats = a.H * a.W;
  const int entries = a.H * C1X3_COLS;

  // weight fragments in registers: [k-step][out tile j][part]
  uint4 wf[5][2][2];
#pragma unroll
  for (int s = 0; s < 5; ++s)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = (2 * ng + j) * 16 + i16;
      const float* src = a.w + ((size_t)co * C1X3_KH + 4 * s + g) * C1X3_KW;
      const f32x4 u = *(const f32x4*)src, v = *(const f32x4*)(src + 4);
      cbf16x8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = e < 4 ? u[e] : v[e - 4];
        h[e] = (__bf16)f;
        l[e] = (__bf16)(f - (float)h[e]);
      }
      wf[s][j][0] = __builtin_bit_cast(uint4, h);
      wf[s][j][1] = __builtin_bit_cast(uint4, l);
    }
  float bias[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[j][r] = a.bias[(2 * ng + j) * 16 + 4 * g + r];

  // the lane's A-fragment byte offset (hi plane, k-step 0) for m-tile mt
  auto aoff = [&](int mt) {
    const int q = 4 * mt + (i16 >> 2), mem = i16 & 3;
    const int ph = q / a.PW, pw = q - ph * a.PW;
    const int r = 2 * ph + (mem >> 1) + g, c = 2 * pw + (mem & 1);
    return (r * C1X3_COLS + ((c + 8 * r) & (C1X3_COLS - 1))) * 16;
  };
  typedef uint4 AFr[5][2];
  auto loadA = [&](AFr& A, int off) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      A[s][0] = *(const uint4*)(img + off + s * 4 * C1X3_COLS * 16);
      A[s][1] = *(const uint4*)(img + C1X3_PLANE + off + s * 4 * C1X3_COLS * 16);
    }
  };
  auto tile = [&](const AFr& A, int mt, __bf16* ob) {
    f32x4 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] = f32x4{bias[j][0], bias[j][1], bias[j][2], bias[j][3]};
#pragma unroll
    for (int s = 0; s < 5; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cbf16x8, wf[s][j][t == 2 ? 1 : 0]),
                                                           __builtin_bit_cast(cbf16x8, A[s][t == 1 ? 1 : 0]),
                                                           acc[j], 0, 0, 0);
    const int q = 4 * mt + (i16 >> 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x4c hv, lv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = relu_nan(acc[j][r]);
        v = nanmax(v, __shfl_xor(v, 1));
        v = nanmax(v, __shfl_xor(v, 2));
        hv[r] = (__bf16)v;
        lv[r] = (__bf16)(v - (float)hv[r]);
      }
      if ((i16 & 3) == 0) {
        __bf16* px = ob + (size_t)q * 128 + (2 * ng + j) * 16 + 4 * g;
        *(bf16x4c*)px = hv;
        *(bf16x4c*)(px + 64) = lv;
      }
    }
  };

  // the next clip's raw rows are loaded into registers while this clip computes
  // (NE entries of 8 floats per thread), converted and written at its start
  constexpr int NE = (C1X3_HMAX * C1X3_COLS + 511) / 512;
  f32x4 pu[NE], pv[NE];
  auto fetch = [&](int bb) {
    const bool ok = bb < a.B;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + (size_t)(ok ? bb : 0) * clip_floats), (short)0, ok ? clip_floats * 4 : 0, 0x00020000);
#pragma unroll
    for (int n = 0; n < NE; ++n) {
      const int e = tid + n * 512;
      const int r = e / C1X3_COLS, c = e - r * C1X3_COLS;
      const int o = e < entries ? (r * a.W + c) * 4 : 0x40000000;
      pu[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
      pv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o + 16, 0, 0));
    }
  };
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();  // every wave is done with the previous clip's image
    fetch(b);
#pragma unroll
    for (int n = 0; n < NE; ++n) {
      const int e = tid + n * 512;
      if (e >= entries) break;
      const int r = e / C1X3_COLS, c = e - r * C1X3_COLS;
      const f32x4 u = pu[n], v = pv[n];
      cbf16x8 h, l;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float f = k < 4 ? u[k] : v[k - 4];
        h[k] = (__bf16)f;
        l[k] = (__bf16)(f - (float)h[k]);
      }
      const int slot = (r * C1X3_COLS + ((c + 8 * r) & (C1X3_COLS - 1))) * 16;
      *(cbf16x8*)(img + slot) = h;
      *(cbf16x8*)(img + C1X3_PLANE + slot) = l;
    }
    __syncthreads();
    __bf16* ob = a.out + (size_t)b * a.PH * a.PW * 128;
    AFr A0, A1;
    int mt = mg;
    if (mt < nmt) loadA(A0, aoff(mt));
    while (mt < nmt) {
      const int m1 = mt + 4;
      if (m1 < nmt) loadA(A1, aoff(m1));
      tile(A0, mt, ob);
      if (m1 >= nmt) break;
      const int m2 = m1 + 4;
      if (m2 < nmt) loadA(A0, aoff(m2));
      tile(A1, m1, ob);
      mt = m2;
    }
  }
}

// ---------------------------------------------------------------------------- //
// conv1 + ReLU + MaxPool2d(2,2) of cnn-trad-pool2 in fp32 (the conv1x3_kernel
// design on v_mfma_f32_16x16x4_f32), writing conv2f_kernel's NHWC fp32 input.
// One clip per tile, 8 waves = 2 n-groups x 4 m-groups.  K = 160 = 10 chunks of
// 16: lane group g of chunk s holds kh = 2s + (g >> 1), kw = 4 (g & 1) + e for
// MFMA e = 0..3.  The clip is staged as a "shifted-row" image of 16-B entries,
// entry (r, c) = x[r][c .. c+3] (c = 0 .. 35), so an operand read is ONE 16-B
// read feeding 4 MFMAs per out tile; the weights W[co][kh][4 (g & 1) .. +3] are 16
// contiguous bytes of the OIHW tensor, held in VGPRs for the launch.  M order
// (pooled pixel, 2x2 member): ReLU, two lane-swap maxes, one 16-B store per lane
// group.  The next clip's rows load into registers during this clip's MFMAs.
// ---------------------------------------------------------------------------- //
constexpr int C1F_COLS = 36;  // entries per image row (the pooled region's 32 columns + kw 0..7 in runs of 4)

struct Conv1FArgs {
  const float* x;     // [B][H][W]
  const float* w;     // [64][1][20][8]
  const float* bias;  // [64]
  float* out;         // [B][PH][PW][64]
  int B, H, W, PH, PW;
};

__global__ __launch_bounds__(512, 1) void conv1f_kernel(Conv1FArgs a) {
  __shared__ __attribute__((aligned(16))) char img[C1X3_HMAX * C1F_COLS * 16];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave & 1, mg = wave >> 1;
  const int g = lane >> 4, i16 = lane & 15;
  const int nmt = a.PH * a.PW / 4;  // 16-row m-tiles of pooled members (host-checked: PH*PW % 4 == 0)
  const int clip_floats = a.H * a.W;
  const int entries = a.H * C1F_COLS;

  f32x4 wf[10][2];
#pragma unroll
  for (int s = 0; s < 10; ++s)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = (2 * ng + j) * 16 + i16;
      wf[s][j] = *(const f32x4*)(a.w + ((size_t)co * C1X3_KH + 2 * s + (g >> 1)) * C1X3_KW + 4 * (g & 1));
    }
  float bias[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[j][r] = a.bias[(2 * ng + j) * 16 + 4 * g + r];

  // the lane's entry offset at chunk 0 for m-tile mt (chunk s adds 2 rows)
  auto aoff = [&](int mt) {
    const int q = 4 * mt + (i16 >> 2), mem = i16 & 3;
    const int ph = q / a.PW, pw = q - ph * a.PW;
    const int r = 2 * ph + (mem >> 1) + (g >> 1), c = 2 * pw + (mem & 1) + 4 * (g & 1);
    return (r * C1F_COLS + c) * 16;
  };
  typedef f32x4 BFr[10];
  auto loadB = [&](BFr& Bv, int off) {
#pragma unroll
    for (int s = 0; s < 10; ++s) Bv[s] = *(const f32x4*)(img + off + s * 2 * C1F_COLS * 16);
  };
  auto tile = [&](const BFr& Bv, int mt, float* ob) {
    f32x4 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] = f32x4{bias[j][0], bias[j][1], bias[j][2], bias[j][3]};
#pragma unroll
    for (int s = 0; s < 10; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s][j][e], Bv[s][e], acc[j], 0, 0, 0);
    const int q = 4 * mt + (i16 >> 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t = relu_nan(acc[j][r]);
        t = nanmax(t, __shfl_xor(t, 1));
        v[r] = nanmax(t, __shfl_xor(t, 2));
      }
      if ((i16 & 3) == 0) *(f32x4*)(ob + (size_t)q * 64 + (2 * ng + j) * 16 + 4 * g) = v;
    }
  };

  constexpr int NE = (C1X3_HMAX * C1F_COLS + 511) / 512;
  f32x4 pu[NE];
  auto fetch = [&](int bb) {
    const bool ok = bb < a.B;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.x + (size_t)(ok ? bb : 0) * clip_floats), (short)0, ok ? clip_floats * 4 : 0, 0x00020000);
#pragma unroll
    for (int n = 0; n < NE; ++n) {
      const int e = tid + n * 512;
      const int r = e / C1F_COLS, c = e - r * C1F_COLS;
      const int o = e < entries ? (r * a.W + c) * 4 : 0x40000000;
      pu[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
    }
  };
  fetch(blockIdx.x);
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();  // every wave is done with the previous clip's image
#pragma unroll
    for (int n = 0; n < NE; ++n) {
      const int e = tid + n * 512;
      if (e < entries) *(f32x4*)(img + e * 16) = pu[n];
    }
    __syncthreads();
    fetch(b + gridDim.x);  // the next clip's rows, landing during this clip's MFMAs
    float* ob = a.out + (size_t)b * a.PH * a.PW * 64;
    BFr B0, B1;
    int mt = mg;
    if (mt < nmt) loadB(B0, aoff(mt));
    while (mt < nmt) {
      const int m1 = mt + 4;
      if (m1 < nmt) loadB(B1, aoff(m1));
      tile(B0, mt, ob);
      if (m1 >= nmt) break;
      const int m2 = m1 + 4;
      if (m2 < nmt) loadB(B0, aoff(m2));
      tile(B1, m1, ob);
      mt = m2;
    }
  }
}

#include "cnn_split.inc"  // the latency schedule's kernels: the four convs above cut into small tiles, split-K Linear

// conv1 in fp32 with conv2f following: trad-pool2's conv1 geometry
static bool conv1f_applies(const honk_cnn_desc* d, int oh1, int ph1, int pw1) {
  if (const char* e = getenv("HONK_CNN_C1F"))
    if (atoi(e) == 0) return false;
  return d->c1_kh == C1X3_KH && d->c1_kw == C1X3_KW && d->c1_sh == 1 && d->c1_sw == 1 && d->c1_out == 64 &&
         2 * pw1 + 4 <= C1F_COLS && d->width >= C1F_COLS + 3 && d->height <= C1X3_HMAX && (ph1 * pw1) % 4 == 0 &&
         oh1 >= 2 * ph1;
}

// conv1 on the fast path: bf16x3 with conv2x3 following, trad-pool2's conv1
// geometry (20 x 8 filter, stride 1, 64 maps, 2x2 pool, 32 pooled-window columns)
static bool conv1x3_applies(const honk_cnn_desc* d, int oh1, int ph1, int pw1) {
  if (const char* e = getenv("HONK_CNN_C1X3"))
    if (atoi(e) == 0) return false;
  return d->c1_kh == C1X3_KH && d->c1_kw == C1X3_KW && d->c1_sh == 1 && d->c1_sw == 1 && d->c1_out == 64 &&
         2 * pw1 == C1X3_COLS && d->width >= C1X3_COLS + C1X3_KW - 1 && d->height <= C1X3_HMAX &&
         (ph1 * pw1) % 4 == 0 && oh1 >= 2 * ph1;
}

// cnn-trad-pool2-class conv2 on the fast path: bf16x3, conv1 pooled 2x2 with 64
// maps (its GEMM writes the NHWC split input), conv2 64 -> <= 64, stride 1, no
// pool after it, an even tap count, a half image within C2X3_IMG and OH*OW
// within the instantiated 2 * 13 m-tiles
constexpr int C2X3_MT = 13;
static bool conv2x3_applies(const honk_cnn_desc* d, int ph1, int pw1, int oh2, int ow2) {
  if (d->precision != HONK_PREC_BF16X3 || !d->has_conv2) return false;
  if (const char* e = getenv("HONK_CNN_C2X3"))
    if (atoi(e) == 0) return false;
  return d->p1_h == 2 && d->p1_w == 2 && d->c1_out == 64 && d->c2_out <= 64 && d->c2_sh == 1 && d->c2_sw == 1 &&
         d->p2_h == 1 && d->p2_w == 1 && (d->c2_kh * d->c2_kw) % 2 == 0 && ph1 * pw1 * 128 <= C2X3_IMG &&
         oh2 * ow2 > 16 * C2X3_MT && oh2 * ow2 <= 32 * C2X3_MT;
}
static size_t conv2x3_frag_bytes(const honk_cnn_desc* d) { return (size_t)2 * d->c2_kh * d->c2_kw * 4 * 2 * 64 * 16; }
// the fp32 counterpart (conv2f_kernel): the same geometry in HONK_PREC_F32
constexpr int C2F_MT = 13;
static bool conv2f_applies(const honk_cnn_desc* d, int ph1, int pw1, int oh2, int ow2) {
  if (d->precision != HONK_PREC_F32 || !d->has_conv2) return false;
  if (const char* e = getenv("HONK_CNN_C2F"))
    if (atoi(e) == 0) return false;
  return d->p1_h == 2 && d->p1_w == 2 && d->c1_out == 64 && d->c2_out <= 64 && d->c2_sh == 1 && d->c2_sw == 1 &&
         d->p2_h == 1 && d->p2_w == 1 && ph1 * pw1 * 128 <= C2X3_IMG && oh2 * ow2 > 16 * C2F_MT &&
         oh2 * ow2 <= 32 * C2F_MT;
}
static size_t conv2f_frag_bytes(const honk_cnn_desc* d) { return (size_t)2 * d->c2_kh * d->c2_kw * 2 * 4 * 64 * 16; }

// gridDim.x of conv_gemm_kernel: one workgroup per BM GEMM rows
static int64_t gemm_grid_x(int64_t M) { return cdiv(M, BM); }

static int launch_gemm(const GemmArgs& a, bool pool2, hipStream_t st, bool x3 = false) {
  if (a.M <= 0 || a.N <= 0) return HONK_OK;
  const int64_t gm = gemm_grid_x(a.M);
  if (gm > 0x7fffffff) return fail(HONK_ERR_ARG, "GEMM too large (M=%lld)", (long long)a.M);
  dim3 grid((unsigned)gm, (unsigned)cdiv(a.N, BN));
  TimedLaunch tl(st, 2.0 * (double)a.M * a.N * a.K);
  if (pool2 && x3)
    hipLaunchKernelGGL((conv_gemm_kernel<true, true>), grid, dim3(256), 0, st, a);
  else if (pool2)
    hipLaunchKernelGGL((conv_gemm_kernel<true, false>), grid, dim3(256), 0, st, a);
  else if (x3)
    hipLaunchKernelGGL((conv_gemm_kernel<false, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_gemm_kernel<false, false>), grid, dim3(256), 0, st, a);
  tl.done(st);
  HONK_LAUNCH_CHECK("conv_gemm_kernel");
  return HONK_OK;
}

static int conv(const float* in, const float* w, const float* bias, float* out, int64_t batch, int cin,
                int h, int wd, int cout, int kh, int kw, int sh, int sw, int relu, hipStream_t st,
                bool pool2 = false, bool x3 = false, int nhwc_x3 = 0, int dil = 1) {
  if ((kh - 1) * dil + 1 > h || (kw - 1) * dil + 1 > wd || sh < 1 || sw < 1 || cin < 1 || cout < 1 || dil < 1)
    return fail(HONK_ERR_ARG, "bad conv geometry (cin=%d %dx%d k=%dx%d s=%dx%d)", cin, h, wd, kh, kw, sh, sw);
  GemmArgs a;
  a.in = in; a.w = w; a.bias = bias; a.out = out;
  a.Cin = cin; a.H = h; a.W = wd; a.KH = kh; a.KW = kw; a.SH = sh; a.SW = sw;
  a.DH = a.DW = dil;
  a.OH = (h - (kh - 1) * dil - 1) / sh + 1;
  a.OW = (wd - (kw - 1) * dil - 1) / sw + 1;
  a.PH = a.OH / 2;
  a.PW = a.OW / 2;
  a.M = pool2 ? batch * a.PH * a.PW * 4 : batch * a.OH * a.OW;
  a.N = cout;
  a.K = cin * kh * kw;
  a.relu = relu;
  a.nhwc_x3 = nhwc_x3;
  if (pool2 && (a.PH < 1 || a.PW < 1)) return fail(HONK_ERR_ARG, "pool larger than conv output");
  return launch_gemm(a, pool2, st, x3);
}

// Linear with few outputs (n <= NB, e.g. cnn-trad-pool2's 26624 -> 4 output
// layer): a GEMV per clip, HBM-bound on x.  One 256-thread block per CPB clips
// walks K with 16-byte loads, every W element read once per block (L2-resident)
// and reused for the CPB clips; wave shuffles + LDS finish the reduction.  The
// GEMM kernel would give such a layer only ceil(m / 128) blocks with the whole
// K serial in each.
template <int NB, int CPB>
__global__ __launch_bounds__(256) void linear_small_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ y,
                                                           int64_t m, int K, int N, int relu) {
  __shared__ float red[4][CPB][NB];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CPB;
  float acc[CPB][NB];
#pragma unroll
  for (int c = 0; c < CPB; ++c)
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[c][n] = 0.f;
  const bool vec = (K & 3) == 0;
  if (vec) {
    const int K4 = K >> 2;
    for (int k4 = tid; k4 < K4; k4 += 256) {
      float4 xv[CPB];
#pragma unroll
      for (int c = 0; c < CPB; ++c)
        xv[c] = (r0 + c < m) ? ((const float4*)(x + (r0 + c) * K))[k4] : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        if (n < N) {
          const float4 wv = ((const float4*)(w + (int64_t)n * K))[k4];
#pragma unroll
          for (int c = 0; c < CPB; ++c)
            acc[c][n] = fmaf(wv.x, xv[c].x, fmaf(wv.y, xv[c].y, fmaf(wv.z, xv[c].z, fmaf(wv.w, xv[c].w, acc[c][n]))));
        }
      }
    }
  } else {
    for (int k = tid; k < K; k += 256) {
      float xv[CPB];
#pragma unroll
      for (int c = 0; c < CPB; ++c) xv[c] = (r0 + c < m) ? x[(r0 + c) * K + k] : 0.f;
#pragma unroll
      for (int n = 0; n < NB; ++n)
        if (n < N) {
          const float wv = w[(int64_t)n * K + k];
#pragma unroll
          for (int c = 0; c < CPB; ++c) acc[c][n] = fmaf(wv, xv[c], acc[c][n]);
        }
    }
  }
#pragma unroll
  for (int c = 0; c < CPB; ++c)
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      float t = acc[c][n];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
      if ((tid & 63) == 0) red[tid >> 6][c][n] = t;
    }
  __syncthreads();
  if (tid < CPB * NB) {
    const int c = tid / NB, n = tid - c * NB;
    if (n < N && r0 + c < m) {
      float v = red[0][c][n] + red[1][c][n] + red[2][c][n] + red[3][c][n] + (b ? b[n] : 0.f);
      if (relu) v = relu_nan(v);
      y[(r0 + c) * N + n] = v;
    }
  }
}

// the kernel a Linear of n outputs runs on (HONK_CNN_KERNEL_*)
static int linear_kind(int n, bool x3) {
  if (n <= 4) return HONK_CNN_KERNEL_LINEAR_SMALL4;
  if (n <= 8) return HONK_CNN_KERNEL_LINEAR_SMALL8;
  if (n <= 16) return HONK_CNN_KERNEL_LINEAR_SMALL16;
  return x3 ? HONK_CNN_KERNEL_LINEAR_GEMM_X3 : HONK_CNN_KERNEL_LINEAR_GEMM_F32;
}

static int linear(const float* x, const float* w, const float* b, float* y, int64_t m, int k, int n,
                  int relu, hipStream_t st, bool x3 = false) {
  const int kind = linear_kind(n, x3);
  if (kind <= HONK_CNN_KERNEL_LINEAR_SMALL16 && m > 0) {
    constexpr int CPB = 4;
    const unsigned blocks = (unsigned)cdiv(m, CPB);
    if (kind == HONK_CNN_KERNEL_LINEAR_SMALL4)
      hipLaunchKernelGGL((linear_small_kernel<4, CPB>), dim3(blocks), dim3(256), 0, st, x, w, b, y, m, k, n, relu);
    else if (kind == HONK_CNN_KERNEL_LINEAR_SMALL8)
      hipLaunchKernelGGL((linear_small_kernel<8, CPB>), dim3(blocks), dim3(256), 0, st, x, w, b, y, m, k, n, relu);
    else
      hipLaunchKernelGGL((linear_small_kernel<16, CPB>), dim3(blocks), dim3(256), 0, st, x, w, b, y, m, k, n, relu);
    HONK_LAUNCH_CHECK("linear_small_kernel");
    return HONK_OK;
  }
  return conv(x, w, b, y, m, k, 1, 1, n, 1, 1, 1, 1, relu, st, false, x3);
}

static int maxpool(const float* in, float* out, int64_t planes, int h, int w, int kh, int kw, hipStream_t st) {
  if (kh < 1 || kw < 1 || kh > h || kw > w) return fail(HONK_ERR_ARG, "bad pool %dx%d on %dx%d", kh, kw, h, w);
  const int64_t total = planes * (h / kh) * (w / kw);
  if (total == 0) return HONK_OK;
  hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, in, out, planes, h, w,
                     kh, kw);
  HONK_LAUNCH_CHECK("maxpool_kernel");
  return HONK_OK;
}


// ---------------------------------------------------------------------------- //
// SpeechModel training (utils/train.py:123-135 on the cnn configs: the backward of
// model.py:186-193).  The forward reuses conv_gemm_kernel (conv + bias + ReLU,
// pre-pool output kept for the backward) and maxpool_kernel; dropout stays
// PyTorch's own op between them (the reference's RNG stream and mask semantics).
//   * max-pool backward: the gradient of each window goes to its first maximum in
//     scan order (the forward's rule, v > m || isnan(v): torch's max_pool2d index);
//   * weight + bias gradient: dW[n][k] = sum_m g'[n][m] X[k][m], k = (ci, kh, kw),
//     m = (clip, oh, ow), g' = the output gradient through the ReLU (act > 0), X
//     gathered from the NCHW input (the forward's im2col), on fp32 MFMA with m as
//     the reduction; the m range is split over workgroups (one partial each) and
//     the partials are summed in a fixed order: deterministic;
//   * input gradient (stride 1): the full correlation of g' with the flipped,
//     transposed weights = conv_gemm_kernel over g' zero-padded by (KH-1, KW-1).
// ---------------------------------------------------------------------------- //
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ in, const float* __restrict__ gout,
                                                          float* __restrict__ gin, int64_t planes, int H, int W,
                                                          int KH, int KW) {
  const int PH = H / KH, PW = W / KW;
  const int64_t total = planes * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int64_t t = i / W;
    const int y = (int)(t % H);
    const int64_t pl = t / H;
    const int ph = y / KH, pw = x / KW;
    float g = 0.f;
    if (ph < PH && pw < PW) {
      const float* p = in + pl * H * W + (int64_t)(ph * KH) * W + pw * KW;
      float m = p[0];
      int best = 0;
      for (int u = 0; u < KH; ++u)
        for (int v = 0; v < KW; ++v) {
          const float e = p[u * W + v];
          if (e > m || e != e) {
            m = e;
            best = u * KW + v;
          }
        }
      if (best == (y - ph * KH) * KW + (x - pw * KW)) g = gout[(pl * PH + ph) * PW + pw];
    }
    gin[i] = g;
  }
}

constexpr int WG_BN = 64;  // out channels per workgroup
constexpr int WG_BK = 64;  // (ci, kh, kw) columns per workgroup
constexpr int WG_BM = 32;  // reduction (m) per LDS stage

struct ConvWgradArgs {
  const float* in;   // [B][Cin][H][W]
  const float* gy;   // [B][N][OH][OW]
  const float* act;  // [B][N][OH][OW] ReLU output (g' = act <= 0 ? 0 : gy), or nullptr
  float* part;       // [S][N][K]
  float* pbias;      // [S][N] or nullptr
  int64_t M, mper;   // B*OH*OW; m per split (multiple of WG_BM)
  int N, K, Cin, H, W, KH, KW, SH, SW, OH, OW;
  int D;             // dilation
};

// 256 threads = 4 waves; wave w owns out channels n0 + 16w .. +15 and all 4
// 16-column tiles of the workgroup's 64 k (4 accumulators).  A stage stages 32 m
// of g' ([m][n]) and X ([m][k]) in LDS, the next stage's global loads in flight
// during the 8 k-steps of v_mfma_f32_16x16x4_f32.  Staging: thread = m column
// (tid & 31) x 8 rows (tid >> 5) + 8j, one (clip, pixel) decomposition per stage.
__global__ __launch_bounds__(256) void conv_wgrad_kernel(ConvWgradArgs a) {
  __shared__ float Gs[2][WG_BM][WG_BN + 4];
  __shared__ float Xs[2][WG_BM][WG_BK + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * WG_BN, k0 = blockIdx.y * WG_BK, sp = blockIdx.z;
  const int64_t mbeg = (int64_t)sp * a.mper;
  const int64_t mend = mbeg + a.mper < a.M ? mbeg + a.mper : a.M;
  const int mc = tid & 31, r8 = tid >> 5;
  const int KHW = a.KH * a.KW, OHW = a.OH * a.OW;
  int koff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + r8 + 8 * j;
    if (k < a.K) {
      const int ci = k / KHW, rem = k - ci * KHW;
      const int kh = rem / a.KW, kw = rem - kh * a.KW;
      koff[j] = (ci * a.H + kh * a.D) * a.W + kw * a.D;
    } else {
      koff[j] = -1;
    }
  }
  const bool do_bias = a.pbias != nullptr && blockIdx.y == 0;
  float gv[8], xv[8], bsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum[j] = 0.f;
  auto load = [&](int64_t m0) {
    const int64_t m = m0 + mc;
    const bool ok = m < mend;
    int64_t gbase = 0, xbase = 0;
    if (ok) {
      const int64_t b = m / OHW;
      const int pix = (int)(m - b * OHW);
      const int oh = pix / a.OW, ow = pix - oh * a.OW;
      gbase = b * (int64_t)a.N * OHW + pix;
      xbase = b * (int64_t)a.Cin * a.H * a.W + (int64_t)(oh * a.SH) * a.W + ow * a.SW;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = n0 + r8 + 8 * j;
      float g = 0.f;
      if (ok && n < a.N) {
        const int64_t o = gbase + (int64_t)n * OHW;
        g = a.gy[o];
        if (a.act && a.act[o] <= 0.f) g = 0.f;  // threshold_backward: NaN passes
      }
      gv[j] = g;
      xv[j] = (ok && koff[j] >= 0) ? a.in[xbase + koff[j]] : 0.f;
    }
    if (do_bias) {
#pragma unroll
      for (int j = 0; j < 8; ++j) bsum[j] += gv[j];
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Gs[buf][mc][r8 + 8 * j] = gv[j];
      Xs[buf][mc][r8 + 8 * j] = xv[j];
    }
  };
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t nst = mend > mbeg ? (mend - mbeg + WG_BM - 1) / WG_BM : 0;
  if (nst > 0) {
    load(mbeg);
    store(0);
  }
  __syncthreads();
  for (int64_t t = 0; t < nst; ++t) {
    const int buf = (int)(t & 1);
    if (t + 1 < nst) load(mbeg + (t + 1) * WG_BM);
#pragma unroll
    for (int ks = 0; ks < WG_BM / 4; ++ks) {
      const int kk = ks * 4 + (lane >> 4);
      const float av = Gs[buf][kk][wave * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Xs[buf][kk][j * 16 + (lane & 15)], acc[j], 0, 0, 0);
    }
    if (t + 1 < nst) store(buf ^ 1);
    __syncthreads();
  }
  // D[i][jj]: lane holds rows i = (lane >> 4) * 4 + r (out channel), column jj = lane & 15 (k)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = k0 + j * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wave * 16 + (lane >> 4) * 4 + r;
      if (n < a.N && k < a.K) a.part[((int64_t)sp * a.N + n) * a.K + k] = acc[j][r];
    }
  }
  if (do_bias) {
    // the 32 lanes of a half-wave share r8: tree over the m columns
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = bsum[j];
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
      const int n = n0 + r8 + 8 * j;
      if (mc == 0 && n < a.N) a.pbias[(int64_t)sp * a.N + n] = v;
    }
  }
}

// out[i] = sum over s of part[s][i], s ascending (fixed order: deterministic)
__global__ __launch_bounds__(256) void split_sum_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                        int64_t n, int S) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += part[(int64_t)s * n + i];
  out[i] = v;
}

// gp[pl][y][x] = g'[pl][y - (KH-1)][x - (KW-1)] inside the map, else 0 (g' = ReLU-masked gy)
__global__ __launch_bounds__(256) void dgrad_pad_kernel(const float* __restrict__ gy, const float* __restrict__ act,
                                                        float* __restrict__ gp, int64_t planes, int OH, int OW,
                                                        int PHp, int PWp, int KH, int KW) {
  const int64_t total = planes * PHp * PWp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % PWp);
    const int64_t t = i / PWp;
    const int y = (int)(t % PHp);
    const int64_t pl = t / PHp;
    const int oy = y - (KH - 1), ox = x - (KW - 1);
    float g = 0.f;
    if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) {
      const int64_t o = (pl * OH + oy) * OW + ox;
      g = gy[o];
      if (act && act[o] <= 0.f) g = 0.f;
    }
    gp[i] = g;
  }
}

// wf[ci][n][kh][kw] = w[n][ci][KH-1-kh][KW-1-kw]
__global__ __launch_bounds__(256) void flip_weights_kernel(const float* __restrict__ w, float* __restrict__ wf, int N,
                                                           int Cin, int KH, int KW) {
  const int KHW = KH * KW;
  const int64_t total = (int64_t)N * Cin * KHW;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % KHW);
  const int64_t q = i / KHW;
  const int n = (int)(q % N);
  const int ci = (int)(q / N);
  wf[i] = w[((int64_t)n * Cin + ci) * KHW + (KHW - 1 - t)];
}

struct WgradPlanC {
  int tn, tk, S;
  int64_t M, mper;
};
static WgradPlanC wgrad_plan_c(int64_t batch, int cin, int h, int w, int cout, int kh, int kw, int sh, int sw,
                               int dil = 1) {
  WgradPlanC p;
  const int oh = (h - (kh - 1) * dil - 1) / sh + 1, ow = (w - (kw - 1) * dil - 1) / sw + 1;
  p.M = batch * oh * ow;
  p.tn = (int)cdiv(cout, WG_BN);
  p.tk = (int)cdiv((int64_t)cin * kh * kw, WG_BK);
  int64_t S = cdiv(1024, (int64_t)p.tn * p.tk);          // ~4 workgroups per CU
  const int64_t smax = cdiv(p.M, 8 * WG_BM);             // >= 8 stages per split
  if (S > smax) S = smax;
  if (S > 4096) S = 4096;
  if (S < 1) S = 1;
  p.mper = cdiv(cdiv(p.M, S), WG_BM) * WG_BM;
  p.S = (int)cdiv(p.M, p.mper);
  if (p.S < 1) p.S = 1;
  return p;
}

// the launch of an elementwise grid-stride kernel of 256 threads (maxpool_bwd_kernel,
// dgrad_pad_kernel): at most 65536 blocks, each thread going round `passes` times
struct StridePlanC {
  int64_t blocks, passes;
};
static StridePlanC stride_plan_c(int64_t total) {
  StridePlanC p;
  p.blocks = cdiv(total, 256) < 65536 ? cdiv(total, 256) : 65536;
  p.passes = p.blocks > 0 ? cdiv(total, p.blocks * 256) : 0;
  return p;
}

// honk_conv2d_dgrad_f32: the pad geometry, the workspace layout ([gp: g' zero-padded]
// [wf: flipped weights]) and the launches (the call, the byte count and
// honk_conv2d_train_plan read this one)
struct DgradPlanC {
  int oh, ow, php, pwp;  // g' dims; padded by (kh-1, kw-1) on every side
  int64_t np, nw;        // floats of gp (wf starts there) and of wf
  int64_t K, M;          // the GEMM's reduction cout*kh*kw and rows batch*h*w
  StridePlanC pad;       // dgrad_pad_kernel
  int64_t gx;            // conv_gemm_kernel gridDim.x
  bool ktab;             // the GEMM's k->offset table in LDS (else computed per load)
  bool wf_aligned;       // wf 16-byte aligned in a 256-byte-aligned workspace
};
static DgradPlanC dgrad_plan_c(int64_t batch, int cin, int h, int w, int cout, int kh, int kw) {
  DgradPlanC p;
  p.oh = h - kh + 1; p.ow = w - kw + 1;
  p.php = p.oh + 2 * (kh - 1); p.pwp = p.ow + 2 * (kw - 1);
  p.np = batch * cout * (int64_t)p.php * p.pwp;
  p.nw = (int64_t)cout * cin * kh * kw;
  p.K = (int64_t)cout * kh * kw;
  p.M = batch * (int64_t)(p.php - kh + 1) * (p.pwp - kw + 1);
  p.pad = stride_plan_c(p.np);
  p.gx = gemm_grid_x(p.M);
  p.ktab = p.K <= KTAB;
  p.wf_aligned = (p.np * (int64_t)sizeof(float)) % 16 == 0;
  return p;
}


// the weight / bias gradient launches (conv_wgrad_kernel + the fixed-order split sums)
static int wgrad_launch(const float* in, const float* gy, const float* act, float* dw, float* db, int64_t batch,
                        int cin, int h, int w, int cout, int kh, int kw, int sh, int sw, int dil, float* part,
                        hipStream_t st) {
  const int64_t K = (int64_t)cin * kh * kw;
  const WgradPlanC p = wgrad_plan_c(batch, cin, h, w, cout, kh, kw, sh, sw, dil);
  ConvWgradArgs a;
  a.in = in; a.gy = gy; a.act = act;
  a.part = part;
  a.pbias = db ? a.part + (int64_t)p.S * cout * K : nullptr;
  a.M = p.M; a.mper = p.mper;
  a.N = cout; a.K = (int)K; a.Cin = cin; a.H = h; a.W = w; a.KH = kh; a.KW = kw; a.SH = sh; a.SW = sw;
  a.OH = (h - (kh - 1) * dil - 1) / sh + 1; a.OW = (w - (kw - 1) * dil - 1) / sw + 1;
  a.D = dil;
  {
    TimedLaunch tl(st, 2.0 * (double)p.M * cout * K);
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3(p.tn, p.tk, p.S), dim3(256), 0, st, a);
    tl.done(st);
  }
  HONK_LAUNCH_CHECK("conv_wgrad_kernel");
  const int64_t nw = (int64_t)cout * K;
  hipLaunchKernelGGL(split_sum_kernel, dim3((unsigned)cdiv(nw, 256)), dim3(256), 0, st, a.part, dw, nw, p.S);
  if (db)
    hipLaunchKernelGGL(split_sum_kernel, dim3((unsigned)cdiv(cout, 256)), dim3(256), 0, st, a.pbias, db,
                       (int64_t)cout, p.S);
  HONK_LAUNCH_CHECK("split_sum_kernel");
  return HONK_OK;
}

// xp[pl][y][x] = x[pl][y - d][x - d] inside the map, else 0 (the "same" conv's zero padding)
__global__ __launch_bounds__(256) void pad_same_kernel(const float* __restrict__ x, float* __restrict__ xp,
                                                       int64_t planes, int H, int W, int d) {
  const int Hp = H + 2 * d, Wp = W + 2 * d;
  const int64_t total = planes * Hp * Wp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % Wp);
    const int64_t t = i / Wp;
    const int yy = (int)(t % Hp);
    const int64_t pl = t / Hp;
    const int sy = yy - d, sx = xx - d;
    xp[i] = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? x[(pl * H + sy) * W + sx] : 0.f;
  }
}
static int pad_same(const float* x, float* xp, int64_t planes, int h, int w, int d, hipStream_t st) {
  const int64_t total = planes * (int64_t)(h + 2 * d) * (w + 2 * d);
  const int64_t blocks = cdiv(total, 256) < 65536 ? cdiv(total, 256) : 65536;
  hipLaunchKernelGGL(pad_same_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, xp, planes, h, w, d);
  HONK_LAUNCH_CHECK("pad_same_kernel");
  return HONK_OK;
}

struct Shapes {
  int oh1, ow1, ph1, pw1, oh2, ow2, ph2, pw2;
  int64_t a1, p1, a2, p2;  // floats per clip of conv1 / pool1 / conv2 / pool2 outputs
  int flat;
  int64_t vec;  // floats per clip of the largest vector stage
};

static int shapes(const honk_cnn_desc* d, Shapes* s) {
  if (!d) return fail(HONK_ERR_ARG, "null descriptor");
  if (d->height < 1 || d->width < 1 || d->n_labels < 1 || d->c1_out < 1 || d->c1_kh < 1 || d->c1_kw < 1 ||
      d->c1_sh < 1 || d->c1_sw < 1 || d->p1_h < 1 || d->p1_w < 1 || d->c1_kh > d->height || d->c1_kw > d->width)
    return fail(HONK_ERR_ARG, "bad cnn descriptor");
  s->oh1 = (d->height - d->c1_kh) / d->c1_sh + 1;
  s->ow1 = (d->width - d->c1_kw) / d->c1_sw + 1;
  s->ph1 = s->oh1 / d->p1_h;
  s->pw1 = s->ow1 / d->p1_w;
  if (s->ph1 < 1 || s->pw1 < 1) return fail(HONK_ERR_ARG, "pool1 larger than conv1 output");
  s->a1 = (int64_t)d->c1_out * s->oh1 * s->ow1;
  s->p1 = (int64_t)d->c1_out * s->ph1 * s->pw1;
  s->flat = (int)s->p1;
  s->a2 = s->p2 = 0;
  if (d->has_conv2) {
    if (d->c2_out < 1 || d->c2_kh < 1 || d->c2_kw < 1 || d->c2_sh < 1 || d->c2_sw < 1 || d->p2_h < 1 ||
        d->p2_w < 1 || d->c2_kh > s->ph1 || d->c2_kw > s->pw1)
      return fail(HONK_ERR_ARG, "bad conv2 descriptor");
    s->oh2 = (s->ph1 - d->c2_kh) / d->c2_sh + 1;
    s->ow2 = (s->pw1 - d->c2_kw) / d->c2_sw + 1;
    s->ph2 = s->oh2 / d->p2_h;
    s->pw2 = s->ow2 / d->p2_w;
    if (s->ph2 < 1 || s->pw2 < 1) return fail(HONK_ERR_ARG, "pool2 larger than conv2 output");
    s->a2 = (int64_t)d->c2_out * s->oh2 * s->ow2;
    s->p2 = (int64_t)d->c2_out * s->ph2 * s->pw2;
    s->flat = (int)s->p2;
  }
  int64_t v = 32;
  if (d->dnn1 > v) v = d->dnn1;
  if (d->dnn2 > v) v = d->dnn2;
  s->vec = v;
  return HONK_OK;
}

// ping-pong buffers A/B hold the per-stage activations of a chunk of clips
static int64_t per_clip_floats(const Shapes& s) {
  int64_t m = s.a1;
  if (s.p1 > m) m = s.p1;
  if (s.a2 > m) m = s.a2;
  if (s.p2 > m) m = s.p2;
  if (s.vec > m) m = s.vec;
  return m;
}

static int64_t chunk_clips(const Shapes& s, int64_t batch) {
  int64_t ch = (int64_t)((size_t)2 << 30) / (per_clip_floats(s) * 4);  // ~2 GiB per buffer
  if (const char* e = getenv("HONK_CNN_CHUNK")) ch = atoll(e);
  if (ch < 1) ch = 1;
  return batch < ch ? batch : ch;
}

// The forward's launch schedule: the per-call weight pack (L_PACK), then one step per
// launch of a chunk.  honk_cnn_launch_plan / honk_cnn_latency_plan report it, the workspace
// queries size the fragment and partial regions from it and the forwards run it: the
// _applies predicates, the latency threshold and the split geometry are decided here and
// nowhere else.
enum Layer { L_PACK, L_CONV1, L_POOL1, L_CONV2, L_POOL2, L_LIN, L_DNN1, L_DNN2, L_OUT };
struct Step {
  int layer, kind;     // kind: HONK_CNN_KERNEL_*
  int64_t tiles = 0;   // the launch's workgroups for `clips` clips (latency plans; 0 where it was not asked for)
  int aux = 0;         // CONV1XS / CONV1FS: m-tiles per band; LINEAR_SPLITK / _SUM: K slices
  int lds = 0;         // the split convs: LDS bytes of one half image / plane
};
struct Plan {
  Step steps[16];
  int n = 0;
  Step& add(int layer, int kind) {
    steps[n] = Step{layer, kind};
    return steps[n++];
  }
  bool has(int kind) const {
    for (int i = 0; i < n; ++i)
      if (steps[i].kind == kind) return true;
    return false;
  }
};

static int gemm_kind(bool x3, bool pool2, int nhwc_x3) {
  return HONK_CNN_KERNEL_GEMM | (x3 ? HONK_CNN_GEMM_X3 : 0) | (pool2 ? HONK_CNN_GEMM_POOL2 : 0) |
         (nhwc_x3 == 1 ? HONK_CNN_GEMM_NHWC_BF16 : nhwc_x3 == 2 ? HONK_CNN_GEMM_NHWC_F32 : 0);
}

// ---- the latency schedule's decisions ----
// Chunks of fewer clips than this run the split kernels: fewer clips than CUs (a dedicated
// throughput kernel would leave CUs idle), and no more than the largest measured batch at which
// the split schedule was not slower than the throughput one (cnn-trad-pool2
// on an MI355X, 96 clips in fp32 and 64 in bf16x3 -- the one-wave conv2 tiles re-read their
// weight fragments per tile, which the whole-clip kernels amortise over 13 m-tiles)
constexpr int64_t LAT_MAX_BATCH_F32 = 96, LAT_MAX_BATCH_X3 = 64;
static int64_t latency_threshold(int cus, bool x3) {
  const int64_t cap = (x3 ? LAT_MAX_BATCH_X3 : LAT_MAX_BATCH_F32) + 1;
  return cus < cap ? cus : cap;
}

// K slice of the split-K Linear: a function of (K, N) only, never of the batch or the device
// (the sweep); a multiple of 4 so that 16-byte loads stay aligned
constexpr int SK_SLICE = 1024;
static int splitk_slice(int K, int N) {
  (void)K; (void)N;
  int sl = SK_SLICE;
  if (const char* e = getenv("HONK_CNN_SPLITK_SLICE")) sl = atoi(e);  // (the sweep's knob)
  if (sl < 4) sl = 4;
  return (sl + 3) & ~3;
}
// K slices of a Linear on the split-K kernels, or 0: shorter than two slices
static int splitk_slices(int K, int N) {
  const int sl = splitk_slice(K, N);
  return K >= 2 * sl ? (int)cdiv(K, sl) : 0;
}

// conv2, split: LDS bytes of one half image of the tallest tile (16 consecutive output pixels
// span at most 15 / OW + 2 output rows), or 0 where two of them exceed C2S_LDS_MAX
static int conv2s_half_bytes(const honk_cnn_desc* d, const Shapes& s) {
  int rows = 15 / s.ow2 + 2 + d->c2_kh - 1;
  if (rows > s.ph1) rows = s.ph1;
  const int64_t hb = cdiv((int64_t)rows * s.pw1 * 8, 64) * 1024;
  return 2 * hb <= C2S_LDS_MAX ? (int)hb : 0;
}

// conv1, split: rows of the tallest band of bm m-tiles
static int conv1s_rows(const Shapes& s, int bm) {
  const int nmt = s.ph1 * s.pw1 / 4;
  int rows = 0;
  for (int m0 = 0; m0 < nmt; m0 += bm) {
    const int m1 = m0 + bm < nmt ? m0 + bm : nmt;
    const int r = 2 * ((4 * m1 - 1) / s.pw1 - (4 * m0) / s.pw1) + 2 + C1X3_KH - 1;
    if (r > rows) rows = r;
  }
  return rows;
}
constexpr int C1S_LDS_MAX = 64 * 1024;
// m-tiles per band (a multiple of 4: one per wave): the largest that still gives every CU a
// workgroup where the chunk yields that many (bands of 4 m-tiles x 2 n-groups), within the LDS
static int conv1s_band_mtiles(const Shapes& s, int64_t clips, int cus, bool x3) {
  const int nmt = s.ph1 * s.pw1 / 4;
  const int64_t most = clips * cdiv(nmt, 4) * 2;
  const int64_t want = most < cus ? most : cus;
  int bm = 4;
  while (bm + 4 <= ((nmt + 3) & ~3) && clips * cdiv(nmt, bm + 4) * 2 >= want) bm += 4;
  const int per_row = x3 ? 2 * C1X3_COLS * 16 : C1F_COLS * 16;
  while (bm > 4 && conv1s_rows(s, bm) * per_row > C1S_LDS_MAX) bm -= 4;
  return bm;
}

// clips = 0: the throughput plan (tiles not filled).  clips > 0: the plan of a chunk of that
// many clips on a device of `cus` CUs, with tiles; `latency` asks for the latency schedule,
// which is the throughput plan at and above latency_threshold(cus, x3).
static Plan plan_forward(const honk_cnn_desc* d, const Shapes& s, int64_t clips = 0, int cus = 0,
                         bool latency = false) {
  Plan p;
  const bool x3 = d->precision == HONK_PREC_BF16X3;
  const bool split = latency && clips > 0 && clips < latency_threshold(cus, x3);
  const bool c2x3 = conv2x3_applies(d, s.ph1, s.pw1, s.oh2, s.ow2);
  const bool c2f = conv2f_applies(d, s.ph1, s.pw1, s.oh2, s.ow2);
  const int64_t grid = clips < cus ? clips : cus;  // the dedicated throughput kernels' persistent grid
  auto gemm_tiles = [&](int64_t M, int N) { return cdiv(M, BM) * cdiv(N, BN); };
  if (c2x3)  // conv2 weights -> hi/lo fragments
    p.add(L_PACK, HONK_CNN_KERNEL_PACK_CONV2X3).tiles = cdiv(2 * d->c2_kh * d->c2_kw * 4 * 2 * 64 * 8, 256);
  if (c2f)   // conv2 weights -> fp32 fragments
    p.add(L_PACK, HONK_CNN_KERNEL_PACK_CONV2F).tiles = cdiv(2 * d->c2_kh * d->c2_kw * 2 * 4 * 64 * 4, 256);
  // conv1 + ReLU (model.py:187), pool1 (:189; skipped when 1x1)
  const bool fuse1 = d->p1_h == 2 && d->p1_w == 2;  // conv1 + ReLU + MaxPool2d(2,2) in one kernel
  const bool c1f = c2f && conv1f_applies(d, s.oh1, s.ph1, s.pw1);
  const bool c1x3 = !c1f && c2x3 && conv1x3_applies(d, s.oh1, s.ph1, s.pw1);
  if ((c1f || c1x3) && split) {
    Step& st = p.add(L_CONV1, c1f ? HONK_CNN_KERNEL_CONV1FS : HONK_CNN_KERNEL_CONV1XS);
    st.aux = conv1s_band_mtiles(s, clips, cus, c1x3);
    st.lds = conv1s_rows(s, st.aux) * (c1x3 ? C1X3_COLS : C1F_COLS) * 16;
    st.tiles = clips * cdiv(s.ph1 * s.pw1 / 4, st.aux) * 2;
  } else if (c1f || c1x3) {
    p.add(L_CONV1, c1f ? HONK_CNN_KERNEL_CONV1F : HONK_CNN_KERNEL_CONV1X3).tiles = grid;
  } else {
    p.add(L_CONV1, gemm_kind(x3, fuse1, c2x3 ? 1 : c2f ? 2 : 0)).tiles =
        gemm_tiles(fuse1 ? clips * s.ph1 * s.pw1 * 4 : clips * s.oh1 * s.ow1, d->c1_out);
  }
  if (!fuse1 && d->p1_h * d->p1_w > 1) p.add(L_POOL1, HONK_CNN_KERNEL_MAXPOOL).tiles = cdiv(clips * s.p1, 256);
  if (c2x3 || c2f) {  // model.py:190-193 on the fast path (pool2 is 1x1)
    const int hb = conv2s_half_bytes(d, s);
    if (split && hb) {
      Step& st = p.add(L_CONV2, c2x3 ? HONK_CNN_KERNEL_CONV2XS : HONK_CNN_KERNEL_CONV2FS);
      st.lds = hb;
      st.tiles = clips * cdiv(s.oh2 * s.ow2, 16) * cdiv(d->c2_out, 16);
    } else {
      p.add(L_CONV2, c2x3 ? HONK_CNN_KERNEL_CONV2X3 : HONK_CNN_KERNEL_CONV2F).tiles = grid;
    }
  } else if (d->has_conv2) {
    const bool fuse2 = d->p2_h == 2 && d->p2_w == 2;
    p.add(L_CONV2, gemm_kind(x3, fuse2, 0)).tiles =
        gemm_tiles(fuse2 ? clips * s.ph2 * s.pw2 * 4 : clips * s.oh2 * s.ow2, d->c2_out);
    if (!fuse2 && d->p2_h * d->p2_w > 1) p.add(L_POOL2, HONK_CNN_KERNEL_MAXPOOL).tiles = cdiv(clips * s.p2, 256);
  }
  int width = s.flat;
  auto lin = [&](int layer, int n) {
    const int S = split ? splitk_slices(width, n) : 0;
    if (S) {  // a K of at least two slices: one partial per slice, then their sum
      Step& a = p.add(layer, HONK_CNN_KERNEL_LINEAR_SPLITK);
      a.aux = S;
      a.tiles = (int64_t)S * cdiv(clips, SK_ROWS) * cdiv(n, SK_NB);
      Step& b = p.add(layer, HONK_CNN_KERNEL_LINEAR_SPLITK_SUM);
      b.aux = S;
      b.tiles = cdiv(clips * n, 256);
    } else {
      const int kind = linear_kind(n, x3);
      p.add(layer, kind).tiles = kind <= HONK_CNN_KERNEL_LINEAR_SMALL16 ? cdiv(clips, 4) : gemm_tiles(clips, n);
    }
    width = n;
  };
  if (d->has_lin) lin(L_LIN, 32);          // :195-196
  if (d->dnn1) lin(L_DNN1, d->dnn1);       // :197-201
  if (d->dnn2) lin(L_DNN2, d->dnn2);       // :202-204
  lin(L_OUT, d->n_labels);                 // :205
  return p;
}

static size_t frag_bytes(const honk_cnn_desc* d, const Plan& p) {
  return (p.has(HONK_CNN_KERNEL_PACK_CONV2X3) ? conv2x3_frag_bytes(d) : 0) +
         (p.has(HONK_CNN_KERNEL_PACK_CONV2F) ? conv2f_frag_bytes(d) : 0);
}

// floats of the split-K partial region of a chunk of `clips` clips: the largest [S][clips][n]
static int64_t partial_floats(const honk_cnn_desc* d, const Shapes& s, int64_t clips) {
  int64_t m = 0;
  int width = s.flat;
  auto lin = [&](int n) {
    const int64_t f = (int64_t)splitk_slices(width, n) * clips * n;
    if (f > m) m = f;
    width = n;
  };
  if (d->has_lin) lin(32);
  if (d->dnn1) lin(d->dnn1);
  if (d->dnn2) lin(d->dnn2);
  lin(d->n_labels);
  return m;
}

// y = act(x w^T + b) on the split-K kernels, two launches: the S slices' partials into `part`
// ([S][m][n]), then their sum in ascending slice order + bias + ReLU
static int splitk_partials(const float* x, const float* w, float* part, int64_t m, int k, int n, int S,
                           hipStream_t st) {
  if (m <= 0) return HONK_OK;
  const int64_t rg = cdiv(m, SK_ROWS);
  if (rg > 65535 || cdiv(n, SK_NB) > 65535)
    return fail(HONK_ERR_ARG, "split-K Linear too large (m=%lld n=%d)", (long long)m, n);
  hipLaunchKernelGGL(linear_splitk_kernel, dim3((unsigned)S, (unsigned)rg, (unsigned)cdiv(n, SK_NB)), dim3(256), 0, st,
                     x, w, part, m, k, n, splitk_slice(k, n));
  HONK_LAUNCH_CHECK("linear_splitk_kernel");
  return HONK_OK;
}
static int splitk_sum(const float* part, const float* b, float* y, int64_t m, int n, int relu, int S, hipStream_t st) {
  if (m <= 0) return HONK_OK;
  hipLaunchKernelGGL(linear_splitk_sum_kernel, dim3((unsigned)cdiv(m * n, 256)), dim3(256), 0, st, part, b, y, m * n, n,
                     S, relu);
  HONK_LAUNCH_CHECK("linear_splitk_sum_kernel");
  return HONK_OK;
}

}  // namespace cnn
}  // namespace honk

using namespace honk;
using namespace honk::cnn;

extern "C" {

int honk_conv2d_f32(const float* in, const float* w, const float* bias, float* out, int64_t batch, int32_t cin,
                    int32_t h, int32_t w_, int32_t cout, int32_t kh, int32_t kw, int32_t sh, int32_t sw,
                    int32_t relu, void* stream) {
  if (!in || !w || !out) return fail(HONK_ERR_ARG, "null pointer argument");
  return conv(in, w, bias, out, batch, cin, h, w_, cout, kh, kw, sh, sw, relu, (hipStream_t)stream);
}

int honk_maxpool2d_f32(const float* in, float* out, int64_t batch, int32_t c, int32_t h, int32_t w, int32_t kh,
                       int32_t kw, void* stream) {
  if (!in || !out) return fail(HONK_ERR_ARG, "null pointer argument");
  return maxpool(in, out, batch * c, h, w, kh, kw, (hipStream_t)stream);
}

int honk_linear_f32(const float* x, const float* w, const float* b, float* y, int64_t m, int32_t k, int32_t n,
                    int32_t relu, void* stream) {
  if (k < 1 || n < 1 || m < 0) return fail(HONK_ERR_ARG, "bad linear shape");
  if (m == 0) return HONK_OK;
  if (!x || !w || !y) return fail(HONK_ERR_ARG, "null pointer argument");
  return linear(x, w, b, y, m, k, n, relu, (hipStream_t)stream);
}

int honk_maxpool2d_bwd_f32(const float* in, const float* gout, float* gin, int64_t batch, int32_t c, int32_t h,
                           int32_t w, int32_t kh, int32_t kw, void* stream) {
  if (!in || !gout || !gin) return fail(HONK_ERR_ARG, "null pointer argument");
  if (batch < 0 || c < 1 || kh < 1 || kw < 1 || kh > h || kw > w)
    return fail(HONK_ERR_ARG, "bad pool %dx%d on %dx%d", kh, kw, h, w);
  const int64_t total = batch * c * h * w;
  if (total == 0) return HONK_OK;
  const StridePlanC p = stride_plan_c(total);
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)p.blocks), dim3(256), 0, (hipStream_t)stream, in, gout, gin,
                     batch * c, h, w, kh, kw);
  HONK_LAUNCH_CHECK("maxpool_bwd_kernel");
  return HONK_OK;
}

int honk_maxpool2d_bwd_plan(int64_t batch, int32_t c, int32_t h, int32_t w, int32_t kh, int32_t kw, int64_t* out,
                            int32_t n_out) {
  if (n_out < 0 || (n_out > 0 && !out)) return fail(HONK_ERR_ARG, "bad plan buffer");
  if (batch < 0 || c < 1 || kh < 1 || kw < 1 || kh > h || kw > w)
    return fail(HONK_ERR_ARG, "bad pool %dx%d on %dx%d", kh, kw, h, w);
  const StridePlanC p = stride_plan_c(batch * c * h * w);
  const int64_t v[HONK_MAXPOOL2D_BWD_PLAN_COUNT] = {p.blocks, p.passes};
  for (int i = 0; i < n_out && i < HONK_MAXPOOL2D_BWD_PLAN_COUNT; ++i) out[i] = v[i];
  return HONK_MAXPOOL2D_BWD_PLAN_COUNT;
}

// what honk_conv2d_wgrad_f32 takes; dgrad: what honk_conv2d_dgrad_f32 takes on top (the
// GEMM's reduction is cout*kh*kw there)
static int conv_train_check(int64_t batch, int cin, int h, int w, int cout, int kh, int kw, int sh, int sw,
                            bool dgrad = false) {
  if (batch < 0 || cin < 1 || cout < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || kh > h || kw > w)
    return fail(HONK_ERR_ARG, "bad conv geometry (cin=%d %dx%d k=%dx%d s=%dx%d cout=%d)", cin, h, w, kh, kw, sh, sw,
                cout);
  // the kernels index k = (ci, kh, kw) in an int; conv_wgrad_kernel's gridDim.y is tk
  const int64_t khw = (int64_t)kh * kw;
  const int64_t kmax = dgrad ? 0x7fffffff : (int64_t)65535 * WG_BK;
  const int chan = dgrad ? cout : cin;
  if (khw > kmax || chan * khw > kmax)
    return fail(HONK_ERR_UNSUPPORTED, "conv training: %s*kh*kw = %d*%d*%d too large (up to %lld)",
                dgrad ? "cout" : "cin", chan, kh, kw, (long long)kmax);
  return HONK_OK;
}

size_t honk_conv2d_wgrad_workspace_bytes(int64_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh,
                                         int32_t kw, int32_t sh, int32_t sw) {
  if (batch < 1 || conv_train_check(batch, cin, h, w, cout, kh, kw, sh, sw) != HONK_OK) return 0;
  const WgradPlanC p = wgrad_plan_c(batch, cin, h, w, cout, kh, kw, sh, sw);
  return (size_t)p.S * ((size_t)cout * cin * kh * kw + cout) * sizeof(float);
}

int honk_conv2d_train_plan(int64_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh, int32_t kw,
                           int32_t sh, int32_t sw, int64_t* out, int32_t n_out) {
  if (n_out < 0 || (n_out > 0 && !out)) return fail(HONK_ERR_ARG, "bad plan buffer");
  int rc = conv_train_check(batch, cin, h, w, cout, kh, kw, sh, sw);
  if (rc) return rc;
  if (batch < 1) return fail(HONK_ERR_ARG, "conv training plan: batch %lld", (long long)batch);
  int64_t v[HONK_CONV2D_TRAIN_PLAN_COUNT] = {0};
  const WgradPlanC p = wgrad_plan_c(batch, cin, h, w, cout, kh, kw, sh, sw);
  v[HONK_CONV2D_TRAIN_PLAN_M] = p.M;
  v[HONK_CONV2D_TRAIN_PLAN_TN] = p.tn;
  v[HONK_CONV2D_TRAIN_PLAN_TK] = p.tk;
  v[HONK_CONV2D_TRAIN_PLAN_S] = p.S;
  v[HONK_CONV2D_TRAIN_PLAN_MPER] = p.mper;
  if (sh == 1 && sw == 1) {
    rc = conv_train_check(batch, cin, h, w, cout, kh, kw, 1, 1, true);
    if (rc) return rc;
    const DgradPlanC q = dgrad_plan_c(batch, cin, h, w, cout, kh, kw);
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_K] = q.K;
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_KTAB] = q.ktab;
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_WF_ALIGNED] = q.wf_aligned;
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_GRID_X] = q.gx;
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_PAD_BLOCKS] = q.pad.blocks;
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_PAD_PASSES] = q.pad.passes;
    v[HONK_CONV2D_TRAIN_PLAN_DGRAD_M] = q.M;
  }
  for (int i = 0; i < n_out && i < HONK_CONV2D_TRAIN_PLAN_COUNT; ++i) out[i] = v[i];
  return HONK_CONV2D_TRAIN_PLAN_COUNT;
}

int honk_conv2d_wgrad_f32(const float* in, const float* gy, const float* act, float* dw, float* db, int64_t batch,
                          int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh, int32_t kw, int32_t sh,
                          int32_t sw, void* workspace, size_t ws_bytes, void* stream) {
  int rc = conv_train_check(batch, cin, h, w, cout, kh, kw, sh, sw);
  if (rc) return rc;
  if (!in || !gy || !dw) return fail(HONK_ERR_ARG, "null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t K = (int64_t)cin * kh * kw;
  if (batch == 0) {
    HONK_HIP_CHECK(hipMemsetAsync(dw, 0, (size_t)cout * K * sizeof(float), st));
    if (db) HONK_HIP_CHECK(hipMemsetAsync(db, 0, (size_t)cout * sizeof(float), st));
    return HONK_OK;
  }
  const size_t need = honk_conv2d_wgrad_workspace_bytes(batch, cin, h, w, cout, kh, kw, sh, sw);
  if (!workspace || ws_bytes < need) return fail(HONK_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  return wgrad_launch(in, gy, act, dw, db, batch, cin, h, w, cout, kh, kw, sh, sw, 1, (float*)workspace, st);
}

size_t honk_conv2d_dgrad_workspace_bytes(int64_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t kh,
                                         int32_t kw) {
  if (batch < 1 || conv_train_check(batch, cin, h, w, cout, kh, kw, 1, 1, true) != HONK_OK) return 0;
  const DgradPlanC p = dgrad_plan_c(batch, cin, h, w, cout, kh, kw);
  return (size_t)(p.np + p.nw) * sizeof(float);
}

int honk_conv2d_dgrad_f32(const float* gy, const float* act, const float* w, float* dx, int64_t batch, int32_t cin,
                          int32_t h, int32_t w_, int32_t cout, int32_t kh, int32_t kw, void* workspace,
                          size_t ws_bytes, void* stream) {
  int rc = conv_train_check(batch, cin, h, w_, cout, kh, kw, 1, 1, true);
  if (rc) return rc;
  if (!gy || !w || !dx) return fail(HONK_ERR_ARG, "null pointer argument");
  if (batch == 0) return HONK_OK;
  const size_t need = honk_conv2d_dgrad_workspace_bytes(batch, cin, h, w_, cout, kh, kw);
  if (!workspace || ws_bytes < need) return fail(HONK_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const DgradPlanC p = dgrad_plan_c(batch, cin, h, w_, cout, kh, kw);
  float* gp = (float*)workspace;
  float* wf = gp + p.np;
  hipLaunchKernelGGL(dgrad_pad_kernel, dim3((unsigned)p.pad.blocks), dim3(256), 0, st, gy, act, gp, batch * cout,
                     p.oh, p.ow, p.php, p.pwp, kh, kw);
  HONK_LAUNCH_CHECK("dgrad_pad_kernel");
  hipLaunchKernelGGL(flip_weights_kernel, dim3((unsigned)cdiv(p.nw, 256)), dim3(256), 0, st, w, wf, cout, cin, kh, kw);
  HONK_LAUNCH_CHECK("flip_weights_kernel");
  return conv(gp, wf, nullptr, dx, batch, cout, p.php, p.pwp, cin, kh, kw, 1, 1, 0, st);
}

// ---- the res block conv for any channel count (model.py:94-98: 3x3, padding =
// dilation = d, no bias), the training kernels' general path: the input zero-padded
// into the workspace, then the implicit GEMM with dilation ----
static int same_check(const void* a, const void* b, const void* c, int64_t batch, int32_t ch, int32_t h, int32_t w,
                      int32_t d) {
  if (!a || !b || !c) return fail(HONK_ERR_ARG, "null pointer argument");
  if (batch < 0 || ch < 1 || h < 1 || w < 1 || d < 1 || d > 1024)
    return fail(HONK_ERR_ARG, "bad same-conv shape (B=%lld C=%d H=%d W=%d d=%d)", (long long)batch, ch, h, w, d);
  if ((int64_t)ch * 9 > 0x7fffffff / 4) return fail(HONK_ERR_UNSUPPORTED, "same-conv: C=%d too large", ch);
  return HONK_OK;
}

size_t honk_conv_same_workspace_bytes(int64_t batch, int32_t c, int32_t h, int32_t w_, int32_t dil) {
  if (batch < 1 || c < 1 || h < 1 || w_ < 1 || dil < 1) return 0;
  const int hp = h + 2 * dil, wp = w_ + 2 * dil;
  const size_t pad = (size_t)batch * c * hp * wp;
  const WgradPlanC p = wgrad_plan_c(batch, c, hp, wp, c, 3, 3, 1, 1, dil);
  size_t extra = (size_t)p.S * c * c * 9;
  if ((size_t)c * c * 9 > extra) extra = (size_t)c * c * 9;
  return (pad + extra) * sizeof(float);
}

int honk_conv_same_f32(const float* x, const float* w, float* y, int64_t batch, int32_t c, int32_t h, int32_t w_,
                       int32_t dil, int32_t flip, void* workspace, size_t ws_bytes, void* stream) {
  int rc = same_check(x, w, y, batch, c, h, w_, dil);
  if (rc) return rc;
  if (batch == 0) return HONK_OK;
  const size_t need = honk_conv_same_workspace_bytes(batch, c, h, w_, dil);
  if (!workspace || ws_bytes < need) return fail(HONK_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int hp = h + 2 * dil, wp = w_ + 2 * dil;
  float* xp = (float*)workspace;
  float* wf = xp + (size_t)batch * c * hp * wp;
  rc = pad_same(x, xp, batch * c, h, w_, dil, st);
  if (rc) return rc;
  const float* wk = w;
  if (flip) {  // input gradient: the flipped, transposed kernel, w'[i][o][t] = w[o][i][8 - t]
    const int64_t nw = (int64_t)c * c * 9;
    hipLaunchKernelGGL(flip_weights_kernel, dim3((unsigned)cdiv(nw, 256)), dim3(256), 0, st, w, wf, c, c, 3, 3);
    HONK_LAUNCH_CHECK("flip_weights_kernel");
    wk = wf;
  }
  return conv(xp, wk, nullptr, y, batch, c, hp, wp, c, 3, 3, 1, 1, 0, st, false, false, 0, dil);
}

int honk_conv_same_wgrad_f32(const float* x, const float* dy, float* dw, int64_t batch, int32_t c, int32_t h,
                             int32_t w_, int32_t dil, void* workspace, size_t ws_bytes, void* stream) {
  int rc = same_check(x, dy, dw, batch, c, h, w_, dil);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {
    HONK_HIP_CHECK(hipMemsetAsync(dw, 0, (size_t)c * c * 9 * sizeof(float), st));
    return HONK_OK;
  }
  const size_t need = honk_conv_same_workspace_bytes(batch, c, h, w_, dil);
  if (!workspace || ws_bytes < need) return fail(HONK_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  const int hp = h + 2 * dil, wp = w_ + 2 * dil;
  float* xp = (float*)workspace;
  float* part = xp + (size_t)batch * c * hp * wp;
  rc = pad_same(x, xp, batch * c, h, w_, dil, st);
  if (rc) return rc;
  return wgrad_launch(xp, dy, nullptr, dw, nullptr, batch, c, hp, wp, c, 3, 3, 1, 1, dil, part, st);
}

size_t honk_cnn_workspace_bytes(const honk_cnn_desc* d, int64_t batch) {
  Shapes s;
  if (shapes(d, &s) != HONK_OK || batch < 1) return 0;
  return (size_t)2 * chunk_clips(s, batch) * per_clip_floats(s) * sizeof(float) + frag_bytes(d, plan_forward(d, s));
}

// the latency schedule's workspace: the throughput one (activations, fragments) + the split-K partials
static size_t latency_partial_bytes(const honk_cnn_desc* d, const Shapes& s, int64_t chunk) {
  return (size_t)partial_floats(d, s, chunk < LAT_MAX_BATCH_F32 ? chunk : LAT_MAX_BATCH_F32) * sizeof(float);
}

size_t honk_cnn_latency_workspace_bytes(const honk_cnn_desc* d, int64_t batch) {
  Shapes s;
  if (shapes(d, &s) != HONK_OK || batch < 1) return 0;
  return honk_cnn_workspace_bytes(d, batch) + latency_partial_bytes(d, s, chunk_clips(s, batch));
}

static int check_precision(const honk_cnn_desc* d) {
  if (d->precision != HONK_PREC_F32 && d->precision != HONK_PREC_BF16X3)
    return fail(HONK_ERR_UNSUPPORTED, "cnn path precision %d (f32 or bf16x3)", d->precision);
  return HONK_OK;
}

int honk_cnn_launch_plan(const honk_cnn_desc* d, int32_t* kinds, int32_t max_kinds) {
  Shapes s;
  int rc = shapes(d, &s);
  if (rc) return rc;
  rc = check_precision(d);
  if (rc) return rc;
  const Plan p = plan_forward(d, s);
  for (int k = 0; kinds && k < p.n && k < max_kinds; ++k) kinds[k] = p.steps[k].kind;
  return p.n;
}

int64_t honk_cnn_latency_threshold(const honk_cnn_desc* d, int32_t n_cus) {
  if (!d) return fail(HONK_ERR_ARG, "null descriptor");
  const int rc = check_precision(d);
  if (rc) return rc;
  if (n_cus < 0) return fail(HONK_ERR_ARG, "negative CU count");
  return latency_threshold(n_cus > 0 ? n_cus : cu_count(), d->precision == HONK_PREC_BF16X3);
}

int honk_cnn_latency_plan(const honk_cnn_desc* d, int64_t batch, int32_t n_cus, int32_t* kinds, int64_t* tiles,
                          int32_t max_steps) {
  Shapes s;
  int rc = shapes(d, &s);
  if (rc) return rc;
  rc = check_precision(d);
  if (rc) return rc;
  if (batch < 1 || n_cus < 0) return fail(HONK_ERR_ARG, "latency plan of %lld clips on %d CUs", (long long)batch, n_cus);
  const Plan p = plan_forward(d, s, chunk_clips(s, batch), n_cus > 0 ? n_cus : cu_count(), true);
  for (int k = 0; k < p.n && k < max_steps; ++k) {
    if (kinds) kinds[k] = p.steps[k].kind;
    if (tiles) tiles[k] = p.steps[k].tiles;
  }
  return p.n;
}

int32_t honk_linear_splitk_slices(int32_t k, int32_t n) {
  if (k < 1 || n < 1) return 0;
  return splitk_slices(k, n);
}

size_t honk_linear_splitk_workspace_bytes(int64_t m, int32_t k, int32_t n) {
  if (m < 1 || k < 1 || n < 1) return 0;
  return (size_t)cdiv(k, splitk_slice(k, n)) * m * n * sizeof(float);
}

int honk_linear_splitk_f32(const float* x, const float* w, const float* b, float* y, int64_t m, int32_t k, int32_t n,
                           int32_t relu, void* workspace, size_t ws_bytes, void* stream) {
  if (k < 1 || n < 1 || m < 0) return fail(HONK_ERR_ARG, "bad linear shape");
  if (m == 0) return HONK_OK;
  if (!x || !w || !y) return fail(HONK_ERR_ARG, "null pointer argument");
  const size_t need = honk_linear_splitk_workspace_bytes(m, k, n);
  if (!workspace || ws_bytes < need) return fail(HONK_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  // (a K shorter than two slices, which the forward keeps on its throughput kernel, runs here as well)
  const int S = (int)cdiv(k, splitk_slice(k, n));
  int rc = splitk_partials(x, w, (float*)workspace, m, k, n, S, (hipStream_t)stream);
  if (rc) return rc;
  return splitk_sum((const float*)workspace, b, y, m, n, relu, S, (hipStream_t)stream);
}

// Both forwards and honk_cnn_features_f32: the checks, the per-call weight pack, then per chunk
// the steps of its plan (latency: the plan of that chunk's clips on this device).  `features`
// (logits NULL): stop before the first Linear and copy the flattened NCHW conv output out.
static int run_forward(const honk_cnn_desc* d, const float* const* t, const float* x, float* logits, float* features,
                       int64_t batch, void* workspace, size_t ws_bytes, void* stream, bool latency) {
  Shapes s;
  int rc = shapes(d, &s);
  if (rc) return rc;
  if (batch < 0) return fail(HONK_ERR_ARG, "negative batch");
  if (batch == 0) return HONK_OK;
  if (!t || !x || !(logits || features) || !workspace) return fail(HONK_ERR_ARG, "null pointer argument");
  if (!t[0] || !t[1] || !t[10] || !t[11]) return fail(HONK_ERR_ARG, "conv1/output tensors are required");
  if (d->has_conv2 && (!t[2] || !t[3])) return fail(HONK_ERR_ARG, "conv2 tensors missing");
  if (d->has_lin && (!t[4] || !t[5])) return fail(HONK_ERR_ARG, "lin tensors missing");
  if (d->dnn1 && (!t[6] || !t[7])) return fail(HONK_ERR_ARG, "dnn1 tensors missing");
  if (d->dnn2 && (!t[8] || !t[9])) return fail(HONK_ERR_ARG, "dnn2 tensors missing");
  if (d->dnn2 && !d->dnn1) return fail(HONK_ERR_ARG, "dnn2 without dnn1");
  const Plan base = plan_forward(d, s);  // (the pack steps and the fragment region are the same in both schedules)
  const int64_t chunk = chunk_clips(s, batch);
  const size_t act = (size_t)2 * chunk * per_clip_floats(s) * sizeof(float) + frag_bytes(d, base);
  const size_t need = act + (latency ? latency_partial_bytes(d, s, chunk) : 0);
  if (ws_bytes < need) return fail(HONK_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  rc = check_precision(d);
  if (rc) return rc;
  const bool x3 = d->precision == HONK_PREC_BF16X3;
  hipStream_t st = (hipStream_t)stream;
  float* A = (float*)workspace;
  float* B = A + chunk * per_clip_floats(s);
  uint4* c2frag = (uint4*)(B + chunk * per_clip_floats(s));
  float* part = (float*)((char*)workspace + act);
  const int ntap = d->c2_kh * d->c2_kw;
  for (int i = 0; i < base.n; ++i) {  // one small launch per call
    if (base.steps[i].kind == HONK_CNN_KERNEL_PACK_CONV2X3) {
      const int total = 2 * ntap * 4 * 2 * 64 * 8;
      hipLaunchKernelGGL(pack_conv2x3_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, t[2],
                         (__bf16*)c2frag, d->c2_out, ntap);
      HONK_LAUNCH_CHECK("pack_conv2x3_kernel");
    } else if (base.steps[i].kind == HONK_CNN_KERNEL_PACK_CONV2F) {
      const int total = 2 * ntap * 2 * 4 * 64 * 4;
      hipLaunchKernelGGL(pack_conv2f_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, t[2], (float*)c2frag,
                         d->c2_out, ntap);
      HONK_LAUNCH_CHECK("pack_conv2f_kernel");
    }
  }

  for (int64_t c0 = 0; c0 < batch; c0 += chunk) {
    const int64_t n = (batch - c0 < chunk) ? batch - c0 : chunk;
    if (n > 0x7fffffff) return fail(HONK_ERR_ARG, "chunk too large");
    const Plan plan = latency ? plan_forward(d, s, n, cu_count(), true) : base;
    const unsigned grid = (unsigned)(n < cu_count() ? n : cu_count());  // the dedicated kernels' persistent grid
    // ping-pong: every step reads cur and writes other (conv1: x -> A); flatten is free: NCHW (model.py:194)
    const float* cur = x + c0 * d->height * d->width;
    float* other = A;
    int width = s.flat;
    auto wrote = [&]() {  // a step's output is the next one's input
      cur = other;
      other = (cur == A) ? B : A;
    };
    // a Linear step: its throughput kernel, or one of the split-K pair (the partials leave cur in place)
    auto lin_step = [&](const Step& sp, const float* w, const float* b, float* y, int nout, int relu) {
      if (sp.kind == HONK_CNN_KERNEL_LINEAR_SPLITK) return splitk_partials(cur, w, part, n, width, nout, sp.aux, st);
      const int r = sp.kind == HONK_CNN_KERNEL_LINEAR_SPLITK_SUM ? splitk_sum(part, b, y, n, nout, relu, sp.aux, st)
                                                                 : linear(cur, w, b, y, n, width, nout, relu, st, x3);
      width = nout;
      return r;
    };
    for (int i = 0; i < plan.n; ++i) {
      const Step& sp = plan.steps[i];
      const int kind = sp.kind;
      const bool gemm = (kind & HONK_CNN_KERNEL_GEMM) != 0;
      const bool pool = gemm && (kind & HONK_CNN_GEMM_POOL2);
      if (features && sp.layer >= L_LIN) break;
      rc = HONK_OK;
      switch (sp.layer) {
        case L_PACK:
          continue;
        case L_CONV1:
          if (kind == HONK_CNN_KERNEL_CONV1F) {
            Conv1FArgs c;
            c.x = cur; c.w = t[0]; c.bias = t[1]; c.out = other;
            c.B = (int)n; c.H = d->height; c.W = d->width; c.PH = s.ph1; c.PW = s.pw1;
            TimedLaunch tl(st, 2.0 * (double)n * s.ph1 * s.pw1 * 4 * 64 * C1X3_KH * C1X3_KW);
            hipLaunchKernelGGL(conv1f_kernel, dim3(grid), dim3(512), 0, st, c);
            tl.done(st);
            HONK_LAUNCH_CHECK("conv1f_kernel");
          } else if (kind == HONK_CNN_KERNEL_CONV1X3) {
            Conv1X3Args c;
            c.x = cur; c.w = t[0]; c.bias = t[1]; c.out = (__bf16*)other;
            c.B = (int)n; c.H = d->height; c.W = d->width; c.PH = s.ph1; c.PW = s.pw1;
            TimedLaunch tl(st, 2.0 * (double)n * s.ph1 * s.pw1 * 4 * 64 * C1X3_KH * C1X3_KW);
            hipLaunchKernelGGL(conv1x3_kernel, dim3(grid), dim3(512), 0, st, c);
            tl.done(st);
            HONK_LAUNCH_CHECK("conv1x3_kernel");
          } else if (kind == HONK_CNN_KERNEL_CONV1FS || kind == HONK_CNN_KERNEL_CONV1XS) {
            const bool xs = kind == HONK_CNN_KERNEL_CONV1XS;
            Conv1SArgs c;
            c.x = cur; c.w = t[0]; c.bias = t[1]; c.out = other;
            c.B = (int)n; c.H = d->height; c.W = d->width; c.PH = s.ph1; c.PW = s.pw1;
            c.bm = sp.aux; c.nbands = (int)cdiv(s.ph1 * s.pw1 / 4, sp.aux); c.plane = sp.lds;
            TimedLaunch tl(st, 2.0 * (double)n * s.ph1 * s.pw1 * 4 * 64 * C1X3_KH * C1X3_KW);
            if (xs)
              hipLaunchKernelGGL(conv1xs_kernel, dim3((unsigned)sp.tiles), dim3(256), 2 * sp.lds, st, c);
            else
              hipLaunchKernelGGL(conv1fs_kernel, dim3((unsigned)sp.tiles), dim3(256), sp.lds, st, c);
            tl.done(st);
            HONK_LAUNCH_CHECK("conv1 split kernel");
          } else {
            rc = conv(cur, t[0], t[1], other, n, 1, d->height, d->width, d->c1_out, d->c1_kh, d->c1_kw, d->c1_sh,
                      d->c1_sw, 1, st, pool, x3,
                      (kind & HONK_CNN_GEMM_NHWC_BF16) ? 1 : (kind & HONK_CNN_GEMM_NHWC_F32) ? 2 : 0);
          }
          break;
        case L_POOL1:
          rc = maxpool(cur, other, n * d->c1_out, s.oh1, s.ow1, d->p1_h, d->p1_w, st);
          break;
        case L_CONV2:
          if (kind == HONK_CNN_KERNEL_CONV2X3) {  // on the NHWC hi/lo pooled conv1 output
            Conv2X3Args c;
            c.in = (const __bf16*)cur; c.wfrag = c2frag; c.bias = t[3]; c.out = other;
            c.B = (int)n; c.PH = s.ph1; c.PW = s.pw1; c.KW = d->c2_kw; c.ntap = ntap;
            c.OH = s.oh2; c.OW = s.ow2; c.N = d->c2_out;
            TimedLaunch tl(st, 2.0 * (double)n * s.oh2 * s.ow2 * d->c2_out * 64 * ntap);
            hipLaunchKernelGGL((conv2x3_kernel<C2X3_MT>), dim3(grid), dim3(256), 0, st, c);
            tl.done(st);
            HONK_LAUNCH_CHECK("conv2x3_kernel");
          } else if (kind == HONK_CNN_KERNEL_CONV2F) {  // fp32, on the NHWC pooled conv1 output
            Conv2FArgs c;
            c.in = cur; c.wfrag = (const f32x4*)c2frag; c.bias = t[3]; c.out = other;
            c.B = (int)n; c.PH = s.ph1; c.PW = s.pw1; c.KW = d->c2_kw; c.ntap = ntap;
            c.OH = s.oh2; c.OW = s.ow2; c.N = d->c2_out;
            TimedLaunch tl(st, 2.0 * (double)n * s.oh2 * s.ow2 * d->c2_out * 64 * ntap);
            hipLaunchKernelGGL((conv2f_kernel<C2F_MT>), dim3(grid), dim3(256), 0, st, c);
            tl.done(st);
            HONK_LAUNCH_CHECK("conv2f_kernel");
          } else if (kind == HONK_CNN_KERNEL_CONV2XS || kind == HONK_CNN_KERNEL_CONV2FS) {
            Conv2SArgs c;
            c.in = cur; c.wfrag = c2frag; c.bias = t[3]; c.out = other;
            c.B = (int)n; c.PH = s.ph1; c.PW = s.pw1; c.KW = d->c2_kw; c.ntap = ntap;
            c.OH = s.oh2; c.OW = s.ow2; c.N = d->c2_out;
            c.nmt = (int)cdiv(s.oh2 * s.ow2, 16); c.nnt = (int)cdiv(d->c2_out, 16); c.half_bytes = sp.lds;
            TimedLaunch tl(st, 2.0 * (double)n * s.oh2 * s.ow2 * d->c2_out * 64 * ntap);
            if (kind == HONK_CNN_KERNEL_CONV2XS)
              hipLaunchKernelGGL(conv2xs_kernel, dim3((unsigned)sp.tiles), dim3(64), 2 * sp.lds, st, c);
            else
              hipLaunchKernelGGL(conv2fs_kernel, dim3((unsigned)sp.tiles), dim3(64), 2 * sp.lds, st, c);
            tl.done(st);
            HONK_LAUNCH_CHECK("conv2 split kernel");
          } else {
            rc = conv(cur, t[2], t[3], other, n, d->c1_out, s.ph1, s.pw1, d->c2_out, d->c2_kh, d->c2_kw, d->c2_sh,
                      d->c2_sw, 1, st, pool, x3);
          }
          break;
        case L_POOL2:
          rc = maxpool(cur, other, n * d->c2_out, s.oh2, s.ow2, d->p2_h, d->p2_w, st);
          break;
        case L_LIN:
          rc = lin_step(sp, t[4], t[5], other, 32, 0);
          break;
        case L_DNN1:
          rc = lin_step(sp, t[6], t[7], other, d->dnn1, d->dnn1_relu);
          break;
        case L_DNN2:
          rc = lin_step(sp, t[8], t[9], other, d->dnn2, 0);
          break;
        case L_OUT:
          rc = lin_step(sp, t[10], t[11], logits + c0 * d->n_labels, d->n_labels, 0);
          break;
      }
      if (rc) return rc;
      if (kind != HONK_CNN_KERNEL_LINEAR_SPLITK) wrote();
    }
    if (features)
      HONK_HIP_CHECK(hipMemcpyAsync(features + c0 * s.flat, cur, (size_t)n * s.flat * sizeof(float),
                                    hipMemcpyDeviceToDevice, st));
  }
  return HONK_OK;
}

int honk_cnn_forward(const honk_cnn_desc* d, const float* const* t, const float* x, float* logits, int64_t batch,
                     void* workspace, size_t ws_bytes, void* stream) {
  return run_forward(d, t, x, logits, nullptr, batch, workspace, ws_bytes, stream, false);
}

int honk_cnn_forward_latency(const honk_cnn_desc* d, const float* const* t, const float* x, float* logits,
                             int64_t batch, void* workspace, size_t ws_bytes, void* stream) {
  return run_forward(d, t, x, logits, nullptr, batch, workspace, ws_bytes, stream, true);
}

int honk_cnn_features_f32(const honk_cnn_desc* d, const float* const* t, const float* x, float* features,
                          int64_t batch, void* workspace, size_t ws_bytes, void* stream, int32_t latency) {
  return run_forward(d, t, x, nullptr, features, batch, workspace, ws_bytes, stream, latency != 0);
}

}  // extern "C"
