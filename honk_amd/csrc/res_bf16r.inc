// ---------------------------------------------------------------------------- //
// Row-band bf16 / bf16x3 block kernel (block16r_kernel): one res block layer
// (res_bf16.inc: folded input BN, weights-as-A MFMA order, co16 channel runs,
// residual by selection MFMA, deferred epilogue), staged per TILE.
//
// A dilated 3x3 conv couples row h only with rows h - dil and h + dil, so the
// rows of one residue class r = h mod dil form an independent plain-3-row
// problem.  A tile is TH consecutive rows OF ONE CLASS (rows r + (k TH + j) dil,
// j = 0 .. TH-1, full width W); its three row taps read class rows j - 1 .. j + 1,
// so ONE LDS image of TH + 2 rows (the band plus one halo row above and below,
// rows outside the map = zeros from the buffer bounds check) serves all three dy
// taps: tap dy reads row slot j + dy.  Versus three per-dy images of TH rows this
// moves (TH + 2) / (3 TH) of the bytes (5/9 for TH = 3), and the tile needs one
// barrier instead of three (round 1's per-dy-stage kernel: 2.49 -> 2.2 ms per
// 4096-clip res15 bf16x3 launch).
//
// Double-buffered across tiles: during tile t the waves DMA tile t+1's rows into
// the other image (pieces spread over the dy0 k-steps); one counted vmcnt +
// s_barrier at the top of each tile retires them.  The two images are separate
// __shared__ objects and the tile loop is unrolled by two, so every ds_read names
// its image at compile time (the waitcnt pass then never drains an in-flight DMA
// into the other image before an operand read).
//
// VMEM order per tile t (k-steps in thirds):  DMA(t+1) (first), ST(t-1) (second:
// the previous tile's deferred epilogue), RES(t) (last)
//   top of tile t+1: vmcnt <= |ST| + |RES|  -> DMA(t+1) landed (then barrier)
//   second third of tile t+1: vmcnt <= |DMA| -> RES(t) landed (epilogue of t)
// RES(t) is in flight across the loop back-edge, where the register allocator's
// phi copies make the compiler drain every VMEM op (vmcnt(0)) at the top of every
// other tile; loading RES(t) at k-step 0 instead (two register sets, no drain)
// measured 2% slower, so the late schedule stays.
// Pixels with bit 2 of their image index set hold [lo | hi] instead of [hi | lo]
// in the image (bf16x3, 45 maps): spreads a fragment read's 16 lanes over the
// banks (7.8 -> 4.9 LDS cycles per ds_read_b128, simulated for every dilation).
// ---------------------------------------------------------------------------- //

constexpr int G16R_WMAX = 40;  // widest row the staging plan is sized for (res maps are 40, 20, 13 wide)

template <int NT, int MT, int SP>
struct G16R {
  using G = G16<NT, MT, SP>;
  static constexpr int CB = G::CB, NW = G::NW, MP = G::MP, KS = G::KS;
  static constexpr int FIXED = G::BBYTES + G::NCLS * G::CP * 4;  // weights + zero pads + bias classes
  // each image is followed by one zero pixel (CB bytes): out-of-range taps read
  // it for the hi AND the lo part (offset + CP*2 stays inside the pad)
  static constexpr int RPX_LIM = ((160 * 1024 - FIXED) / 2 / CB - 1) & ~3;
  // staged pixels per image: the tile's rows plus two halo rows of the widest map
  static constexpr int RPX = (MP + 2 * G16R_WMAX < RPX_LIM) ? MP + 2 * G16R_WMAX : RPX_LIM;
  static constexpr int AZ = RPX * CB;                // one zero pixel after the image (out-of-range taps)
  static constexpr int ASTRIDE = AZ + CB;
  static constexpr int PIECES = (RPX * CB / 16 + 63) / 64;  // 1 KiB LDS-DMA pieces of a full image
  static constexpr int PPW = (PIECES + NW - 1) / NW;        // per wave (extra slots repeat the last piece)
  static constexpr int LDS = 2 * ASTRIDE + FIXED;
  static_assert(LDS <= 160 * 1024, "row-band kernel LDS plan exceeds 160 KiB");
  // stores per epilogue (last layer: the wave's channel sums, NT 16-B stores per m-tile)
  template <bool LAST> static constexpr int S = LAST ? MT * NT : SP * MT * G::VPS;
  template <bool RES> static constexpr int RL = RES ? SP * MT * G::NRF : 0;     // residual loads per tile
  // k-steps run across the three dy rows (the image holds all of them): chunk
  // c = 4 s + lane group over 3 dy x 3 dx x 2 NT channel chunks, KSA k-steps
  // (14 for 45 maps vs 3 x 5 with per-dy k-steps), the last one holding UGA used
  // lane groups; weight fragments in that order (pack_block16_kernel xdy = 1)
  static constexpr bool SWZ = SP == 2 && NT == 3;  // [lo | hi] swap for pixels with P & 4
  static constexpr int KSA = (18 * NT + 3) / 4;
  static constexpr int UGA = 18 * NT - 4 * (KSA - 1);
  static_assert(NT * ((KSA - 1) * 1024 + UGA * 256) == G::WPART, "row-band weight layout size");
  static constexpr int xfrag(int part, int s, int n) {
    return part * G::WPART + (s < KSA - 1 ? (s * NT + n) * 1024 : (KSA - 1) * NT * 1024 + n * UGA * 256);
  }
  // hook schedule over the tile's KSA k-steps, in thirds: DMA(t+1) pieces in the
  // first, the previous tile's epilogue (after one counted vmcnt) in the second,
  // RES(t) loads in the last
  // (other thirds -- k-steps (3,7), (5,10), (2,8), (6,12) vs (4,9) for 45 maps --
  // measured within 0.7 %)
  static constexpr int T1 = KSA / 3 > 0 ? KSA / 3 : 1;
  static constexpr int T2 = (2 * KSA) / 3 > T1 ? (2 * KSA) / 3 : T1 + 1;
  static_assert(T2 < KSA, "hook thirds");
  static constexpr int kp(int i) { return i * T1 / PPW; }              // k-step of DMA piece i
  static constexpr int ke(int m) { return T1 + m * (T2 - T1) / MT; }   // k-step of m-tile m's epilogue
  static constexpr int kr(int m) { return T2 + m * (KSA - T2) / MT; }  // k-step of m-tile m's RES loads
};

// operands of row-band k-step S (A hi/lo fragments of the wave's m-tiles, weight
// hi/lo fragments of all out-tiles) from LDS into register set `o`
template <int NT, int MT, int SP, int S>
__device__ __forceinline__ void load_ops16r(const char* abuf, const char* bbase,
                                            const int (&aoff)[SP][G16R<NT, MT, SP>::KSA][MT], int lane16, bool gused,
                                            uint4 (&oa)[SP][MT], uint4 (&ob)[SP][NT]) {
  using G = G16<NT, MT, SP>;
  using R = G16R<NT, MT, SP>;
#pragma unroll
  for (int pt = 0; pt < SP; ++pt) {
#pragma unroll
    for (int m = 0; m < MT; ++m) oa[pt][m] = *(const uint4*)(abuf + aoff[pt][S][m]);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      int o;
      if constexpr (S < R::KSA - 1 || R::UGA == 4) o = R::xfrag(pt, S, n) + lane16;
      else o = gused ? R::xfrag(pt, S, n) + lane16 : G::ZW;
      ob[pt][n] = *(const uint4*)(bbase + o);
    }
  }
}

// One row-band k-step: reads the operands of step S + PD while the MFMAs of step
// S run (PD = G16::PD: 1 at two waves per SIMD, 2 at one) (products as in stage16_step), then the per-k-step hook.  Issue priority
// drops half-way through the tile so a wave that is behind on its SIMD catches
// up before the next barrier.
template <int NT, int MT, int SP, int S, typename Hook>
__device__ __forceinline__ void band16_step(const char* abuf, const char* bbase,
                                            const int (&aoff)[SP][G16R<NT, MT, SP>::KSA][MT], int lane16, bool gused,
                                            f32x4 (&acc)[MT][NT], uint4 (&oa)[G16<NT, MT, SP>::PD + 1][SP][MT],
                                            uint4 (&ob)[G16<NT, MT, SP>::PD + 1][SP][NT], Hook& hook) {
  using R = G16R<NT, MT, SP>;
  constexpr int PD = G16<NT, MT, SP>::PD;
  if constexpr (S < R::KSA) {
    uint4 (&ac)[SP][MT] = oa[S % (PD + 1)];
    uint4 (&bc)[SP][NT] = ob[S % (PD + 1)];
    if constexpr (S + PD < R::KSA)
      load_ops16r<NT, MT, SP, S + PD>(abuf, bbase, aoff, lane16, gused, oa[(S + PD) % (PD + 1)],
                                      ob[(S + PD) % (PD + 1)]);
#pragma unroll
    for (int t = 0; t < (SP == 2 ? 3 : 1); ++t)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bc[t == 2 ? SP - 1 : 0][n]),
                                                              __builtin_bit_cast(bf16x8, ac[t == 1 ? SP - 1 : 0][m]),
                                                              acc[m][n], 0, 0, 0);
    hook(KStep<S>{});
    if constexpr (S == R::KSA / 2) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    band16_step<NT, MT, SP, S + 1>(abuf, bbase, aoff, lane16, gused, acc, oa, ob, hook);
  }
}

// host mirror of G16R::RPX (pixels one staging image holds); MT8 = m-tiles per wave
static constexpr int g16r_rpx(int NT, int MT8, int SP) {
  // G16<NT, MT, SP>: MP = 128 * MT8 (8 waves), FIXED = weights + 512 B zero pad + bias classes
  return (128 * MT8 + 2 * G16R_WMAX < (((160 * 1024 - (g16_frag_bytes(NT, SP) + 512 + 16 * 16 * NT * 4)) / 2 /
                                         (32 * NT * SP) - 1) & ~3))
             ? 128 * MT8 + 2 * G16R_WMAX
             : (((160 * 1024 - (g16_frag_bytes(NT, SP) + 512 + 16 * 16 * NT * 4)) / 2 / (32 * NT * SP) - 1) & ~3);
}
// m-tiles per wave of the layer kernel: the largest whose double-buffered image
// plus the layer's weights fit the 160 KiB LDS
static constexpr int g16r_mt(int NT, int SP) {
  return SP == 1 ? (NT == 3 ? 3 : 4) : (NT == 1 ? 4 : NT == 2 ? 2 : 1);
}

// Band geometry of one clip at dilation d (scalar arithmetic, no table): the
// H mod d classes r < rem hold H/d + 1 rows (nb1 bands of TH rows each), the
// others H/d rows (nb0 bands); band bi -> first row h0 = r + k TH d.
struct BandGeo {
  int rem, nb1, nb0, nbc;
};
__host__ __device__ inline BandGeo band_geo(int H, int d, int TH) {
  BandGeo g;
  const int q = H / d;
  g.rem = H - q * d;
  g.nb1 = (q + 1 + TH - 1) / TH;
  g.nb0 = (q + TH - 1) / TH;
  g.nbc = g.rem * g.nb1 + (d - g.rem) * g.nb0;
  return g;
}
__device__ __forceinline__ int band_h0(int bi, int rem, int nb1, int nb0, int TH, int d) {
  int r, k;
  if (bi < rem * nb1) {
    r = bi / nb1;
    k = bi - r * nb1;
  } else {
    const int bj = bi - rem * nb1;
    const int rr = bj / nb0;
    k = bj - rr * nb0;
    r = rem + rr;
  }
  return r + k * TH * d;
}

struct Block16RArgs {
  const __bf16* in;       // [n][H][W][CP*SP] pre-BN input; its BN is folded into bfrag/bias
  const __bf16* res;      // residual (pre-BN) or nullptr
  __bf16* out;            // pre-BN output, or nullptr (last layer)
  const uint4* bfrag;     // weight fragments (layout G16::wfrag)
  const float* bias;      // [16][CP] folded input-BN shift per border class
  float* chsum;           // last layer: [ntiles][NW][MT][CP] channel sums (one per m-tile), else nullptr
  int H, W, dil, TH, nbc, ntiles;  // nbc = tiles (bands) per clip
  int rem, nb1, nb0;               // band geometry (BandGeo)
  LiveRef live;  // bf16x3 (SP 2) only, count may be null: the clips that run, of the launch's ntiles / nbc
};

template <int NT, int MT, int SP, bool LAST, bool RES>
__global__ __launch_bounds__((G16<NT, MT, SP>::NTHREADS), (G16<NT, MT, SP>::NW / 4)) void block16r_kernel(
    Block16RArgs a) {
  using G = G16<NT, MT, SP>;
  using R = G16R<NT, MT, SP>;
  constexpr int NRF = G::NRF;
  __shared__ __attribute__((aligned(16))) char sa0[R::ASTRIDE];
  __shared__ __attribute__((aligned(16))) char sa1[R::ASTRIDE];
  __shared__ __attribute__((aligned(16))) char sb[R::FIXED];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const int i16 = lane & 15;
  const int lane16 = lane * 16;
  const bool gused = g < R::UGA;  // lane group used in the last k-step

  for (int t = tid; t < 2 * (G::CB / 16); t += G::NTHREADS)
    *(uint4*)((t < G::CB / 16 ? sa0 : sa1) + R::AZ + (t % (G::CB / 16)) * 16) = uint4{0, 0, 0, 0};
  for (int i = tid; i < G::ZW / 16; i += G::NTHREADS) *(uint4*)(sb + i * 16) = a.bfrag[i];
  for (int i = tid; i < 32; i += G::NTHREADS) *(uint4*)(sb + G::ZW + i * 16) = uint4{0, 0, 0, 0};
  const float* biasl = (const float*)(sb + G::BBYTES);
  for (int c = tid; c < G::NCLS * G::CP / 4; c += G::NTHREADS)
    ((f32x4*)(sb + G::BBYTES))[c] = ((const f32x4*)a.bias)[c];

  u32x4 idA[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    bf16x8 e;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      e[j] = (co16(NT, n, i16) == 32 * (n >> 1) + 8 * g + j) ? (__bf16)1.0f : (__bf16)0.0f;
    idA[n] = __builtin_bit_cast(u32x4, e);
  }

  const int H = a.H, W = a.W, d = a.dil, TH = a.TH;
  const int TP = TH * W;
  const int RB = W * G::CB;  // bytes of one staged row
  // per m-tile: the lane's band row j and column w (j = -1: pixel past the band)
  int jrow[MT], wcol[MT];
  // per (k-step, m-tile): LDS offset of the lane's A fragment: chunk c = 4 s + g
  // -> row slot j + dy, column w + (dx - 1) dil, 8-channel chunk cc; R::AZ (zeros)
  // outside the row
  // (SWZ) pixels with bit 2 of their image index set hold [lo | hi] instead of
  // [hi | lo]: spreads a fragment read's 16 lanes over the banks (7.8 -> 4.9 LDS
  // cycles per ds_read_b128, simulated for every dilation); part pt's offset per entry
  int aoff[SP][R::KSA][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int p = (wave * MT + m) * 16 + i16;
    const int j = p / W;
    const int w = p - j * W;
    jrow[m] = p < TP ? j : -1;
    wcol[m] = w;
#pragma unroll
    for (int s = 0; s < R::KSA; ++s) {
      const int c = 4 * s + g;
      const int dy = c / (6 * NT), c6 = c - dy * (6 * NT);
      const int dx = c6 / (2 * NT), cc = c6 - dx * (2 * NT);
      const int col = w + (dx - 1) * d;
      const bool ok = (c < 18 * NT) && (p < TP) && (col >= 0) && (col < W);
      const int P = (j + dy) * W + col;
      const bool sw = R::SWZ && (P & 4);
#pragma unroll
      for (int pt = 0; pt < SP; ++pt)
        aoff[pt][s][m] = ok ? P * G::CB + (((pt == 1) != sw) ? G::CP * 2 : 0) + cc * 16 : R::AZ;
    }
  }

  // staging pieces: piece pc = wave + i NW covers 16-B chunks [start, start + 64)
  // of the (TH + 2)-row image (start clamped so the last piece ends at the image end;
  // surplus pieces repeat it); gpack = (row slot << 16) | byte offset in the row
  const int chunks = (TH + 2) * RB / 16;
  int pstart[R::PPW];
  unsigned gpack[R::PPW];
#pragma unroll
  for (int i = 0; i < R::PPW; ++i) {
    const int pc = wave + i * G::NW;
    const int st = min(pc * 64, chunks - 64);
    pstart[i] = __builtin_amdgcn_readfirstlane(st);
    const int c = st + lane;
    const int s = c / (RB / 16);
    int boff = (c - s * (RB / 16)) * 16;  // byte offset in the row of LDS slot c
    if constexpr (R::SWZ) {               // swapped pixel: its LDS hi half holds the global lo half
      const int col = boff / G::CB, within = boff - col * G::CB;
      if (((s * W + col) & 4) != 0) boff = col * G::CB + within + (within < G::CP * 2 ? G::CP * 2 : -G::CP * 2);
    }
    gpack[i] = ((unsigned)s << 16) | (unsigned)boff;
  }

  const int GR = gridDim.x;
  const int bid = blockIdx.x;
  const int lb = ((GR & 7) == 0) ? (bid & 7) * (GR >> 3) + (bid >> 3) : bid;
  int tile = lb;
  // (a device-held clip count -- bf16x3, an ordered re-run round: the tiles of its first clips)
  int ntiles = a.ntiles;
  if constexpr (SP == 2) {
    if (a.live.count) ntiles = live_clips(a.live, a.ntiles / a.nbc) * a.nbc;
  }
  if (tile >= ntiles) return;  // whole workgroup, before any barrier

  const int clip_bytes = H * RB;
  // first row h0 of tile tt (class r, band k): its rows are h0 + j dil
  // (readfirstlane: keeps the clip's buffer resources in SGPRs across the tile
  // loop, where the compiler loses track of their uniformity)
  auto tile_geo = [&](int tt, int& b, int& h0) {
    b = __builtin_amdgcn_readfirstlane(tt / a.nbc);
    h0 = __builtin_amdgcn_readfirstlane(band_h0(tt - b * a.nbc, a.rem, a.nb1, a.nb0, TH, d));
  };
  auto clip_rsrc = [&](const void* t, int b, bool ok) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)(ok ? t : (const void*)a.in) + (size_t)b * clip_bytes),
                                             (short)0, ok ? clip_bytes : 0, 0x00020000);
  };
  // staging source of tile tt: its clip's buffer resource (num_records 0 past the
  // end: every piece reads zeros) and first row
  struct Src {
    __amdgpu_buffer_rsrc_t rs;
    int h0;
  };
  auto tile_src = [&](int tt) {
    const bool valid = tt < ntiles;
    int b = 0, h0 = 0;
    if (valid) tile_geo(tt, b, h0);
    return Src{clip_rsrc(a.in, b, valid), h0};
  };
  // DMA piece i of a tile into image dst
  auto issue_piece = [&](char* dst, const Src& src, int i) {
    const __amdgpu_buffer_rsrc_t rs = src.rs;
    const int h0 = src.h0;
    const int h = h0 + ((int)(gpack[i] >> 16) - 1) * d;
    const unsigned voff = ((unsigned)h < (unsigned)H) ? (unsigned)(h * RB) + (gpack[i] & 0xffffu) : 0x80000000u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + pstart[i] * 16), 16,
                                             voff, 0, 0, 0);
  };
  // lane pixel offsets within its clip for tile tt (0x40000000: dropped / zero)
  auto pixel_offsets = [&](int h0, int (&po)[MT], int (&cls)[MT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int h = h0 + jrow[m] * d;
      const bool ok = jrow[m] >= 0 && h < H;
      po[m] = ok ? (h * W + wcol[m]) * G::CB : 0x40000000;
      cls[m] = (wcol[m] < d ? 4 : 0) | (wcol[m] + d >= W ? 8 : 0) | (h < d ? 1 : 0) | (h + d >= H ? 2 : 0);
    }
  };

  constexpr int NS = R::template S<LAST>;
  constexpr int NRL = R::template RL<RES>;
  const __amdgpu_buffer_rsrc_t nul = clip_rsrc(nullptr, 0, false);
  // prologue: DMA(first tile) -> sa0, then stand-ins for ST(t-1) and RES(t-1)
  // (dropped stores) so the first barrier sees the steady-state vmcnt layout
  __syncthreads();  // weights, bias, zero pads visible (no DMA in flight yet)
  {
    const Src s0 = tile_src(tile);
#pragma unroll
    for (int i = 0; i < R::PPW; ++i) issue_piece(sa0, s0, i);
  }
  constexpr int NSTAND = NS + NRL;  // VMEM ops younger than DMA(t) at the top of tile t
#pragma unroll
  for (int i = 0; i < NSTAND; ++i) __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, nul, 0, i * 8, 0);

  u32x4 rvp[MT][NRF][SP];  // residual runs of the tile whose epilogue is pending
  f32x4 accp[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int f = 0; f < NRF; ++f)
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) rvp[m][f][pt] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int n = 0; n < NT; ++n) accp[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int tprev = -1, bprev = 0;
  int poprev[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) poprev[m] = 0x40000000;

  // epilogue of the previous tile for m-tile M: ReLU, + residual (MFMA), bf16
  // (hi, lo) runs stored; or (last layer) the channel sums
  auto epilogue_m = [&](auto mc, __amdgpu_buffer_rsrc_t out_r) {
    constexpr int M = decltype(mc)::value;
    f32x4 v[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[n][k] = relu_keepnan(accp[M][n][k]);
    if constexpr (RES) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int pt = 0; pt < SP; ++pt)
          v[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, idA[n]),
                                                         __builtin_bit_cast(bf16x8, rvp[M][n >> 1][pt]), v[n], 0, 0, 0);
    }
    if constexpr (LAST) {
      // fused spatial mean: per m-tile, the channel sums of its valid pixels reduced over
      // the 16 pixel lanes by DPP (no LDS): one partial per (tile, wave, m-tile), summed
      // in tail_sum_kernel.  (Per m-tile rather than accumulated over the tile's MT
      // m-tiles: the 12 running sums spilled this kernel at 256 registers -- 102 vs
      // 65 us per res8 launch.)
      const bool valid = poprev[M] != 0x40000000;
      const int tq = tprev < 0 ? 0 : tprev;
      const __amdgpu_buffer_rsrc_t cs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(a.chsum + (((size_t)tq * G::NW + wave) * MT + M) * G::CP), (short)0, tprev < 0 ? 0 : G::CP * 4,
          0x00020000);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        f32x4 c;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = sum16_dpp(valid ? v[n][k] : 0.f);
        const int co = (i16 == 0) ? co16(NT, n, 4 * g) * 4 : 0x40000000;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, c), cs, co, 0, 0);
      }
    } else {
      bf16x4 h[SP][NT];
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          h[0][n][k] = (__bf16)v[n][k];
          if constexpr (SP == 2) h[SP - 1][n][k] = (__bf16)(v[n][k] - (float)h[0][n][k]);
        }
      const int off = poprev[M];
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) {
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr) {
          const u32x2 lo = __builtin_bit_cast(u32x2, h[pt][2 * pr]), hi = __builtin_bit_cast(u32x2, h[pt][2 * pr + 1]);
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, out_r, off + 16 * g,
                                                 64 * pr + pt * G::CP * 2, 0);
        }
        if constexpr (NT & 1)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h[pt][NT - 1]), out_r, off + 8 * g,
                                                64 * (NT / 2) + pt * G::CP * 2, 0);
      }
    }
  };
  auto for_m = [](auto f) {
    f(KStep<0>{});
    if constexpr (MT > 1) f(KStep<1>{});
    if constexpr (MT > 2) f(KStep<2>{});
    if constexpr (MT > 3) f(KStep<3>{});
    if constexpr (MT > 4) f(KStep<4>{});
    if constexpr (MT > 5) f(KStep<5>{});
    if constexpr (MT > 6) f(KStep<6>{});
    if constexpr (MT > 7) f(KStep<7>{});
    static_assert(MT <= 8, "for_m");
  };

  // one tile on image `cur`, next tile's rows DMA'd into `nxt`
  auto run_tile = [&](char* cur, char* nxt) {
    int b, h0, po[MT], cls[MT];
    tile_geo(tile, b, h0);
    pixel_offsets(h0, po, cls);
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = *(const f32x4*)(biasl + cls[m] * G::CP + co16(NT, n, 4 * g));
    const int tnext = tile + GR;

    wait_vmcnt<NS + NRL>();        // DMA(tile) landed (this wave's pieces) ...
    __builtin_amdgcn_s_barrier();  // ... and every wave's; every wave is done with `nxt`
    HONK_SETPRIO_HI();
    {
      const Src sn = tile_src(tnext);
      const __amdgpu_buffer_rsrc_t out_r = clip_rsrc(a.out, __builtin_amdgcn_readfirstlane(bprev),
                                                     !LAST && __builtin_amdgcn_readfirstlane(tprev) >= 0);
      const __amdgpu_buffer_rsrc_t rr = clip_rsrc(a.res, b, RES);
      auto hook = [&](auto sc) {
        constexpr int S = decltype(sc)::value;
        auto res_loads = [&](int m) {
#pragma unroll
          for (int f = 0; f < NRF; ++f) {
            const int o = (f < NT / 2 || g < 2) ? po[m] + 16 * g : 0x40000000;
#pragma unroll
            for (int pt = 0; pt < SP; ++pt) {
              rvp[m][f][pt] =
                  __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, o, 64 * f + pt * G::CP * 2, 0));
            }
          }
        };
        // first third: DMA(t+1) pieces into the other image
#pragma unroll
        for (int i = 0; i < R::PPW; ++i)
          if (R::kp(i) == S) issue_piece(nxt, sn, i);
        // RES(tprev) (and older stores) landed: only the DMA pieces are younger
        if constexpr (S == R::ke(0)) wait_vmcnt<R::PPW>();
        // second third: the previous tile's epilogue
        for_m([&](auto mc) {
          constexpr int M = decltype(mc)::value;
          if constexpr (R::ke(M) == S) epilogue_m(mc, out_r);
        });
        // last third: this tile's residual runs (consumed by its epilogue in the next tile)
        if constexpr (RES) {
#pragma unroll
          for (int m = 0; m < MT; ++m)
            if (R::kr(m) == S) res_loads(m);
        }
      };
      uint4 oa[G::PD + 1][SP][MT], ob[G::PD + 1][SP][NT];
      load_ops16r<NT, MT, SP, 0>(cur, sb, aoff, lane16, gused, oa[0], ob[0]);
      if constexpr (G::PD == 2) load_ops16r<NT, MT, SP, 1>(cur, sb, aoff, lane16, gused, oa[1], ob[1]);
      band16_step<NT, MT, SP, 0>(cur, sb, aoff, lane16, gused, acc, oa, ob, hook);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      poprev[m] = po[m];
#pragma unroll
      for (int n = 0; n < NT; ++n) accp[m][n] = acc[m][n];
    }
    tprev = tile;
    bprev = b;
    tile = tnext;
  };

  while (true) {
    run_tile(sa0, sa1);
    if (tile >= ntiles) break;
    run_tile(sa1, sa0);
    if (tile >= ntiles) break;
  }
  wait_vmcnt<0>();
  {
    const __amdgpu_buffer_rsrc_t out_r = clip_rsrc(a.out, bprev, !LAST);
    for_m([&](auto mc) { epilogue_m(mc, out_r); });
  }
}
