// The kernels of the cnn forward's LATENCY schedule (honk_cnn_forward_latency), included by
// cnn.hip inside honk::cnn.  The hand-scheduled kernels above give one workgroup a whole clip,
// so a batch of B clips keeps B CUs busy.  Here the same layers are cut into many small tiles:
//
//   conv2xs_kernel / conv2fs_kernel   conv2x3_kernel / conv2f_kernel, tile = (clip, one 16-pixel
//                                     m-tile, one 16-channel out tile), one wave per workgroup
//   conv1xs_kernel / conv1fs_kernel   conv1x3_kernel / conv1f_kernel, tile = (clip, band of pooled
//                                     m-tiles, n-group of 2 out tiles), 4 waves per workgroup
//   linear_splitk_kernel + _sum       a Linear for few rows: one partial per K slice, summed in
//                                     ascending slice order by a second launch
//
// Per output element the convs issue the MFMAs of their throughput kernel in its order (half
// outer, tap inner, hi*hi / hi*lo / lo*hi; conv1: bias-initialised accumulator, k-step outer)
// on the same fragments, with the same epilogue: their outputs are bit for bit the same.

// ---------------------------------------------------------------------------- //
// conv2, split.  A workgroup is one wave: m-tile mt (output pixels 16 mt .. +15 of the clip)
// x out tile nt.  It stages only the image rows its pixels reach (their output rows plus
// KH - 1), BOTH 32-channel halves at once (two half images in the throughput kernel's
// layout: 128 B per pixel, 16-B chunks XOR-swizzled by the tile-local pixel), by LDS-DMA,
// and then runs the 2 * ntap k-steps without a barrier.  The weight fragments come from
// L2 through a register ring C2S_AHEAD k-steps deep (one accumulator gives the wave ~100
// cycles of MFMA per k-step, far less than a global load's latency).
// ---------------------------------------------------------------------------- //
constexpr int C2S_AHEAD = 8;           // k-steps (x3) / chunks (f32) of weight fragments in flight
constexpr int C2S_LDS_MAX = 64 * 1024; // both half images of a tile (host-checked)

struct Conv2SArgs {
  const void* in;      // x3: [B][PH][PW][hi 64 | lo 64] bf16; f32: [B][PH][PW][64] fp32 (256 B per pixel)
  const void* wfrag;   // pack_conv2x3_kernel's / pack_conv2f_kernel's fragments
  const float* bias;   // [N]
  float* out;          // [B][N][OH][OW]
  int B, PH, PW, KW, ntap, OH, OW, N;
  int nmt, nnt;        // m-tiles per clip, non-empty out tiles
  int half_bytes;      // LDS bytes of one half image (a multiple of 1 KiB)
};

// the rows tile mt reaches and the lane's tile-local input pixel at tap (0, 0); stages both halves
template <bool X3>
__device__ __forceinline__ int conv2s_stage(const Conv2SArgs& a, char* img, int b, int mt, int lane, int* P0) {
  const int ohw = a.OH * a.OW;
  const int pfirst = mt * 16, plast = min(pfirst + 15, ohw - 1);
  const int r0 = pfirst / a.OW, r1 = plast / a.OW;
  const int rows = r1 - r0 + a.ntap / a.KW;  // + KH - 1
  const int chunks = rows * a.PW * 8;
  const int pieces = (chunks + 63) / 64;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const char*)a.in + ((size_t)b * a.PH + r0) * a.PW * 256), (short)0, rows * a.PW * 256, 0x00020000);
  for (int h = 0; h < 2; ++h)
    for (int pc = 0; pc < pieces; ++pc) {
      // lanes past the last chunk re-load it into slots of the piece nothing reads
      const int L = min(pc * 64 + lane, chunks - 1);
      const int P = L >> 3, c = (L & 7) ^ (P & 7);
      const unsigned voff = X3 ? (unsigned)(P * 256 + (c >> 2) * 128 + h * 64 + (c & 3) * 16)
                               : (unsigned)(P * 256 + h * 128 + c * 16);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs, (__attribute__((address_space(3))) void*)(img + h * a.half_bytes + pc * 1024), 16, voff, 0, 0, 0);
    }
  const int p = min(pfirst + (lane & 15), ohw - 1);  // (a lane past the clip's last pixel: computed, not stored)
  const int oh = p / a.OW, ow = p - oh * a.OW;
  *P0 = (oh - r0) * a.PW + ow;
  return pfirst + (lane & 15);
}

__device__ __forceinline__ void conv2s_store(const Conv2SArgs& a, const f32x4& acc, int b, int nt, int p, int g) {
  const int ohw = a.OH * a.OW;
  if (p < ohw) {
    float* ob = a.out + (size_t)b * a.N * ohw;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nt * 16 + 4 * g + r;
      if (n < a.N) ob[(size_t)n * ohw + p] = relu_nan(acc[r] + a.bias[n]);
    }
  }
}

__global__ __launch_bounds__(64) void conv2xs_kernel(Conv2SArgs a) {
  extern __shared__ __attribute__((aligned(16))) char c2s_img[];
  char* img = c2s_img;
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int nt = blockIdx.x % a.nnt;
  const int mt = (blockIdx.x / a.nnt) % a.nmt;
  const int b = blockIdx.x / (a.nnt * a.nmt);
  const int total = 2 * a.ntap;  // k-steps: (half, tap)
  // weight fragments of k-step s, part pt: wl[(s * 8 + pt) * 64]
  const uint4* wl = (const uint4*)a.wfrag + nt * 2 * 64 + lane;
  // Every global load below is unconditional (indices past the last k-step are clamped to it and
  // their data never used): a load under a branch would make the compiler drain the whole ring at
  // the join, since it could no longer count the loads in flight.
  auto loadW = [&](uint4* Wv, int s) {
    const int sc = min(s, total - 1);
    Wv[0] = wl[(sc * 8 + 0) * 64];
    Wv[1] = wl[(sc * 8 + 1) * 64];
  };
  uint4 Wr[C2S_AHEAD][2];
#pragma unroll
  for (int i = 0; i < C2S_AHEAD; ++i) loadW(Wr[i], i);
  int P0;
  const int p = conv2s_stage<true>(a, img, b, mt, lane, &P0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the image landed
  __syncthreads();
  auto loadA = [&](uint4* A, int s) {
    const int sc = min(s, total - 1);
    const int h = sc >= a.ntap ? 1 : 0, t = sc - h * a.ntap;
    const int kh = t / a.KW;
    const int P = P0 + kh * a.PW + (t - kh * a.KW);
    const int ad = h * a.half_bytes + (((P << 3) + (g ^ (P & 7))) << 4);
    A[0] = *(const uint4*)(img + ad);
    A[1] = *(const uint4*)(img + (ad ^ 64));
  };
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 An[2], Ac[2];
  auto mma = [&](const uint4* Wv) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cbf16x8, Wv[t == 2 ? 1 : 0]),
                                                    __builtin_bit_cast(cbf16x8, Ac[t == 1 ? 1 : 0]), acc, 0, 0, 0);
  };
  loadA(An, 0);
  int s0 = 0;
  for (; s0 + C2S_AHEAD <= total; s0 += C2S_AHEAD) {  // whole rings: no branch
#pragma unroll
    for (int i = 0; i < C2S_AHEAD; ++i) {
      Ac[0] = An[0];
      Ac[1] = An[1];
      loadA(An, s0 + i + 1);
      mma(Wr[i]);
      loadW(Wr[i], s0 + i + C2S_AHEAD);
    }
  }
#pragma unroll
  for (int i = 0; i < C2S_AHEAD - 1; ++i)  // the last total % C2S_AHEAD k-steps: their fragments are in the ring
    if (s0 + i < total) {
      Ac[0] = An[0];
      Ac[1] = An[1];
      loadA(An, s0 + i + 1);
      mma(Wr[i]);
    }
  conv2s_store(a, acc, b, nt, p, g);
}

__global__ __launch_bounds__(64) void conv2fs_kernel(Conv2SArgs a) {
  extern __shared__ __attribute__((aligned(16))) char c2s_img[];
  char* img = c2s_img;
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int nt = blockIdx.x % a.nnt;
  const int mt = (blockIdx.x / a.nnt) % a.nmt;
  const int b = blockIdx.x / (a.nnt * a.nmt);
  const int nch = 2 * a.ntap;   // chunks of one half: (tap, q)
  const int total = 2 * nch;
  const f32x4* wl = (const f32x4*)a.wfrag + nt * 64 + lane;  // chunk c: wl[c * 4 * 64]
  // (unconditional, clamped loads: see conv2xs_kernel)
  auto loadW = [&](int c) { return wl[min(c, total - 1) * 4 * 64]; };
  f32x4 Wr[C2S_AHEAD];
#pragma unroll
  for (int i = 0; i < C2S_AHEAD; ++i) Wr[i] = loadW(i);
  int P0;
  const int p = conv2s_stage<false>(a, img, b, mt, lane, &P0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the image landed
  __syncthreads();
  auto loadB = [&](int c) {
    const int cl = min(c, total - 1);
    const int h = cl >= nch ? 1 : 0, cc = cl - h * nch;
    const int t = cc >> 1, q = cc & 1;
    const int kh = t / a.KW;
    const int P = P0 + kh * a.PW + (t - kh * a.KW);
    return *(const f32x4*)(img + h * a.half_bytes + (((P << 3) + ((4 * q + g) ^ (P & 7))) << 4));
  };
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 Bn = loadB(0), Bc;
  auto mma = [&](const f32x4& Wv) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Wv[e], Bc[e], acc, 0, 0, 0);
  };
  int c0 = 0;
  for (; c0 + C2S_AHEAD <= total; c0 += C2S_AHEAD) {  // whole rings: no branch
#pragma unroll
    for (int i = 0; i < C2S_AHEAD; ++i) {
      Bc = Bn;
      Bn = loadB(c0 + i + 1);
      mma(Wr[i]);
      Wr[i] = loadW(c0 + i + C2S_AHEAD);
    }
  }
#pragma unroll
  for (int i = 0; i < C2S_AHEAD - 1; ++i)  // the last total % C2S_AHEAD chunks
    if (c0 + i < total) {
      Bc = Bn;
      Bn = loadB(c0 + i + 1);
      mma(Wr[i]);
    }
  conv2s_store(a, acc, b, nt, p, g);
}

// ---------------------------------------------------------------------------- //
// conv1 + ReLU + 2x2 pool, split.  A workgroup of 4 waves is (clip, band of bm pooled
// m-tiles, n-group ng: out tiles 2 ng, 2 ng + 1); wave mg takes the band's m-tiles
// mg, mg + 4, ...  The shifted-row image holds only the band's input rows (its pooled
// rows' 2 conv rows each, plus KH - 1), at row pitch and swizzle of the throughput kernel.
// ---------------------------------------------------------------------------- //
struct Conv1SArgs {
  const float* x;     // [B][H][W]
  const float* w;     // [64][1][20][8]
  const float* bias;  // [64]
  void* out;          // x3: [B][PH][PW][hi 64 | lo 64] bf16; f32: [B][PH][PW][64] fp32
  int B, H, W, PH, PW;
  int bm, nbands;     // m-tiles per band, bands per clip
  int plane;          // x3: LDS bytes of one (hi or lo) plane
};

// the band's m-tiles [mt0, mt1) and input rows [rbase, rbase + rows)
__device__ __forceinline__ void conv1s_band(const Conv1SArgs& a, int band, int* mt0, int* mt1, int* rbase, int* rows) {
  const int nmt = a.PH * a.PW / 4;
  *mt0 = band * a.bm;
  *mt1 = min(*mt0 + a.bm, nmt);
  const int ph_lo = (4 * *mt0) / a.PW, ph_hi = (4 * *mt1 - 1) / a.PW;
  *rbase = 2 * ph_lo;
  *rows = 2 * (ph_hi - ph_lo) + 2 + C1X3_KH - 1;
}

__global__ __launch_bounds__(256) void conv1xs_kernel(Conv1SArgs a) {
  extern __shared__ __attribute__((aligned(16))) char c1s_img[];
  char* img = c1s_img;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int mg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i16 = lane & 15;
  const int ng = blockIdx.x & 1;
  const int band = (blockIdx.x >> 1) % a.nbands;
  const int b = (blockIdx.x >> 1) / a.nbands;
  int mt0, mt1, rbase, rows;
  conv1s_band(a, band, &mt0, &mt1, &rbase, &rows);
  const int entries = rows * C1X3_COLS;

  // the band's rows -> shifted-row entries (r, c) = x[rbase + r][c .. c+7] as 8 bf16, hi / lo planes
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.x + ((size_t)b * a.H + rbase) * a.W), (short)0, rows * a.W * 4, 0x00020000);
  for (int e0 = 0; e0 < entries; e0 += 4 * 256) {
    f32x4 pu[4], pv[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int e = e0 + n * 256 + tid;
      const int r = e / C1X3_COLS, c = e - r * C1X3_COLS;
      const int o = e < entries ? (r * a.W + c) * 4 : 0x40000000;
      pu[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
      pv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o + 16, 0, 0));
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int e = e0 + n * 256 + tid;
      if (e < entries) {
        const int r = e / C1X3_COLS, c = e - r * C1X3_COLS;
        cbf16x8 h, l;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float f = k < 4 ? pu[n][k] : pv[n][k - 4];
          h[k] = (__bf16)f;
          l[k] = (__bf16)(f - (float)h[k]);
        }
        const int slot = (r * C1X3_COLS + ((c + 8 * r) & (C1X3_COLS - 1))) * 16;
        *(cbf16x8*)(img + slot) = h;
        *(cbf16x8*)(img + a.plane + slot) = l;
      }
    }
  }

  // weight fragments in registers: [k-step][out tile j][part] (conv1x3_kernel's)
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
  __syncthreads();

  __bf16* ob = (__bf16*)a.out + (size_t)b * a.PH * a.PW * 128;
  for (int mt = mt0 + mg; mt < mt1; mt += 4) {
    const int q = 4 * mt + (i16 >> 2), mem = i16 & 3;
    const int ph = q / a.PW, pw = q - ph * a.PW;
    const int r = 2 * ph + (mem >> 1) + g - rbase, c = 2 * pw + (mem & 1);
    const int off = (r * C1X3_COLS + ((c + 8 * r) & (C1X3_COLS - 1))) * 16;
    uint4 A[5][2];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      A[s][0] = *(const uint4*)(img + off + s * 4 * C1X3_COLS * 16);
      A[s][1] = *(const uint4*)(img + a.plane + off + s * 4 * C1X3_COLS * 16);
    }
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
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x4c hv, lv;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float v = relu_nan(acc[j][rr]);
        v = nanmax(v, __shfl_xor(v, 1));
        v = nanmax(v, __shfl_xor(v, 2));
        hv[rr] = (__bf16)v;
        lv[rr] = (__bf16)(v - (float)hv[rr]);
      }
      if ((i16 & 3) == 0) {
        __bf16* px = ob + (size_t)q * 128 + (2 * ng + j) * 16 + 4 * g;
        *(bf16x4c*)px = hv;
        *(bf16x4c*)(px + 64) = lv;
      }
    }
  }
}

__global__ __launch_bounds__(256) void conv1fs_kernel(Conv1SArgs a) {
  extern __shared__ __attribute__((aligned(16))) char c1s_img[];
  char* img = c1s_img;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int mg = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i16 = lane & 15;
  const int ng = blockIdx.x & 1;
  const int band = (blockIdx.x >> 1) % a.nbands;
  const int b = (blockIdx.x >> 1) / a.nbands;
  int mt0, mt1, rbase, rows;
  conv1s_band(a, band, &mt0, &mt1, &rbase, &rows);
  const int entries = rows * C1F_COLS;

  // entries (r, c) = x[rbase + r][c .. c+3]
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.x + ((size_t)b * a.H + rbase) * a.W), (short)0, rows * a.W * 4, 0x00020000);
  for (int e0 = 0; e0 < entries; e0 += 4 * 256) {
    f32x4 pu[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int e = e0 + n * 256 + tid;
      const int r = e / C1F_COLS, c = e - r * C1F_COLS;
      const int o = e < entries ? (r * a.W + c) * 4 : 0x40000000;
      pu[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int e = e0 + n * 256 + tid;
      if (e < entries) *(f32x4*)(img + e * 16) = pu[n];
    }
  }

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
  __syncthreads();

  float* ob = (float*)a.out + (size_t)b * a.PH * a.PW * 64;
  for (int mt = mt0 + mg; mt < mt1; mt += 4) {
    const int q = 4 * mt + (i16 >> 2), mem = i16 & 3;
    const int ph = q / a.PW, pw = q - ph * a.PW;
    const int r = 2 * ph + (mem >> 1) + (g >> 1) - rbase, c = 2 * pw + (mem & 1) + 4 * (g & 1);
    const int off = (r * C1F_COLS + c) * 16;
    f32x4 Bv[10];
#pragma unroll
    for (int s = 0; s < 10; ++s) Bv[s] = *(const f32x4*)(img + off + s * 2 * C1F_COLS * 16);
    f32x4 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] = f32x4{bias[j][0], bias[j][1], bias[j][2], bias[j][3]};
#pragma unroll
    for (int s = 0; s < 10; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s][j][e], Bv[s][e], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4 v;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float t = relu_nan(acc[j][rr]);
        t = nanmax(t, __shfl_xor(t, 1));
        v[rr] = nanmax(t, __shfl_xor(t, 2));
      }
      if ((i16 & 3) == 0) *(f32x4*)(ob + (size_t)q * 64 + (2 * ng + j) * 16 + 4 * g) = v;
    }
  }
}

// ---------------------------------------------------------------------------- //
// Split-K Linear for few rows: y[r][n] = act(b[n] + sum_k x[r][k] w[n][k]).
// Workgroup (K slice s, row group of SK_ROWS rows, n-group of SK_NB outputs): thread t takes
// the slice's 4-element groups t, t + 256, ..., one fmaf chain per (row, n) over its groups'
// elements, then a fixed tree (wave shuffles, the 4 waves in order) leaves the slice's
// partial in part[s][r][n].  linear_splitk_sum_kernel adds the partials in ascending s, then
// the bias, then the ReLU.  No atomics, no counters; a row's sums do not depend on the rows
// around it, and the unaligned (scalar-load) path associates exactly as the 16-byte one.
// ---------------------------------------------------------------------------- //
constexpr int SK_ROWS = 4, SK_NB = 8;

__global__ __launch_bounds__(256) void linear_splitk_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            float* __restrict__ part, int64_t m, int K, int N,
                                                            int slice) {
  __shared__ float red[4][SK_ROWS][SK_NB];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * SK_ROWS;
  const int n0 = blockIdx.z * SK_NB;
  const int kbeg = s * slice, kend = min(K, kbeg + slice);
  const bool vec = (K & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)w)) & 15) == 0;
  float acc[SK_ROWS][SK_NB];
#pragma unroll
  for (int c = 0; c < SK_ROWS; ++c)
#pragma unroll
    for (int n = 0; n < SK_NB; ++n) acc[c][n] = 0.f;
  auto load4 = [&](const float* p, int k) -> f32x4 {  // p[k .. k+3], zero past kend
    if (vec) return *(const f32x4*)(p + k);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < kend ? p[k + e] : 0.f;
    return v;
  };
  for (int k = kbeg + 4 * tid; k < kend; k += 4 * 256) {
    f32x4 xv[SK_ROWS];
#pragma unroll
    for (int c = 0; c < SK_ROWS; ++c)
      xv[c] = (r0 + c < m) ? load4(x + (r0 + c) * K, k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < SK_NB; ++n) {
      if (n0 + n < N) {
        const f32x4 wv = load4(w + (int64_t)(n0 + n) * K, k);
#pragma unroll
        for (int c = 0; c < SK_ROWS; ++c)
          acc[c][n] = fmaf(wv[0], xv[c][0], fmaf(wv[1], xv[c][1], fmaf(wv[2], xv[c][2], fmaf(wv[3], xv[c][3], acc[c][n]))));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < SK_ROWS; ++c)
#pragma unroll
    for (int n = 0; n < SK_NB; ++n) {
      float t = acc[c][n];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
      if ((tid & 63) == 0) red[tid >> 6][c][n] = t;
    }
  __syncthreads();
  if (tid < SK_ROWS * SK_NB) {
    const int c = tid / SK_NB, n = tid - c * SK_NB;
    if (n0 + n < N && r0 + c < m)
      part[((int64_t)s * m + r0 + c) * N + n0 + n] = ((red[0][c][n] + red[1][c][n]) + red[2][c][n]) + red[3][c][n];
  }
}

// y[i] = act(part[0][i] + part[1][i] + ... (ascending s) + b[i % N])
__global__ __launch_bounds__(256) void linear_splitk_sum_kernel(const float* __restrict__ part,
                                                                const float* __restrict__ b, float* __restrict__ y,
                                                                int64_t total, int N, int S, int relu) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[(int64_t)s * total + i];
  if (b) v += b[i % N];
  if (relu) v = relu_nan(v);
  y[i] = v;
}
