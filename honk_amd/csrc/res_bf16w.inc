// ---------------------------------------------------------------------------- //
// Weight-stationary row-band bf16 / bf16x3 block kernel (block16w_kernel): one
// res block layer, the layer's whole weight operand held in registers.
//
// Why: with the weights in LDS (block16r_kernel) every k-step re-reads NT weight
// fragments per part next to the MT activation fragments -- at MT = 1 (all the
// 160 KiB LDS left for the images at bf16x3) that is 8 ds_read_b128 per 9 MFMAs,
// the LDS array's whole bandwidth, and the tile is 3 rows with a 2-row halo.
// Here one wave per SIMD keeps the layer's weight fragments (KSA k-steps x NT
// out-tiles x SP parts x 4 VGPRs: 336 for 45 maps at bf16x3) in the unified
// VGPR/AGPR file for the whole launch, so an m-tile costs 2 (SP) activation
// reads per 9 MFMAs, and the LDS holds only the two staging images: tiles of
// up to 8 rows (res15, dilation 1).
//
// Geometry (same decomposition as block16r): a tile is TH consecutive rows of one
// dilation class (rows r + (k TH + j) dil, j < TH) of one clip; its three row taps
// read class rows j - 1 .. j + 1, so one image of TH + 2 class rows serves all
// taps.  The image columns are ordered by COLUMN class (w mod dil), each class
// preceded by one zero separator pixel: in that order the dilated conv is a plain
// 3x3 conv (taps at -1 / 0 / +1 image pixels, rows +-RW, RW = W + dil pixels per
// row) and the separators are the column zero padding -- no per-tap validity test
// in the MFMA loop.  Rows outside the map come from the buffer bounds check.
//
// Work split: the tile's ceil(rows x W / 16) m-tiles are dealt to the 4 waves
// round-robin; a wave runs its m-tiles one after another, all KSA k-steps of one
// m-tile (K = 3 dy x 3 dx x CP channels, 8-channel chunks, 4 chunks per
// 16x16x32 k-step) before the next, so only one m-tile's accumulators are live.
// The epilogue of m-tile i (ReLU, + residual, bf16 (hi, lo) split, stores -- or
// the fused channel sums of the last layer) runs under the MFMAs of m-tile i + 1,
// one out-tile and at most one store per k-step from k-step KE on; the
// residual runs of m-tile i + 1 are loaded right after it.
// Every wave runs at least one m-tile per tile (a wave past the tile's m-tiles
// computes a dummy whose stores are dropped) so every wave issues the same VMEM
// pattern: the staging DMA of the NEXT tile in its first m-tile (k-steps 1 ..
// KE - 1), one counted vmcnt + s_barrier at the top of each tile.
// ---------------------------------------------------------------------------- //

// Operand formats of the weight-stationary / pair kernels (template parameter FM):
//   0  bf16:   activations and weights one bf16 each, 1 product             (HONK_PREC_BF16)
//   1  bf16x3: both as bf16 (hi, lo), products hw.hx + hw.lx + lw.hx         (HONK_PREC_BF16X3)
//   2  f16x2:  activations one fp16 (RNE), weights fp16 (hi, lo), products
//              hw.x + lw.x on v_mfma_f32_16x16x32_f16, fp32 accumulation     (HONK_PREC_F16X2)
// SP = activation parts in memory (2 for bf16x3 only), WP = weight parts.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <int FM>
struct ActT {
  using T = __bf16;
  using V4 = bf16x4;
};
template <>
struct ActT<2> {
  using T = _Float16;
  using V4 = f16x4;
};
// element e (0/1: low/high half) of a 32-bit word of a stored activation run, as fp32
template <int FM>
__device__ __forceinline__ float act_dec(unsigned u, int e) {
  if constexpr (FM == 2) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)((e & 1) ? (u >> 16) : (u & 0xffffu)));
  } else {
    return __builtin_bit_cast(float, (e & 1) ? (u & 0xffff0000u) : (u << 16));
  }
}

// v + the residual element e of word u.  f16x2: one v_fma_mix_f32 (the fp16 element
// times 1.0 plus v, in fp32: the product is exact, so this is v + (float)r rounded
// once, bit-for-bit the convert-then-add the compiler emits as two instructions)
template <int FM>
__device__ __forceinline__ float add_res(float v, unsigned u, int e) {
  if constexpr (FM == 2) {
    float out;
    if (e & 1) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(out) : "v"(u), "v"(v));
    else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(out) : "v"(u), "v"(v));
    return out;
  } else {
    return v + act_dec<FM>(u, e);
  }
}

template <int NT, int SP, int FM = (SP == 2 ? 1 : 0)>
struct G16W {
  static_assert(SP == (FM == 1 ? 2 : 1), "activation parts follow the format");
  static constexpr int WP = FM == 0 ? 1 : 2;  // weight parts
  static constexpr int CP = 16 * NT;
  static constexpr int CB = CP * 2 * SP;  // bytes per pixel (SP = 2: [hi CP][lo CP] bf16)
  static constexpr int NW = 4;            // waves (one per SIMD)
  static constexpr int NTHREADS = 64 * NW;
  static constexpr int KSA = (18 * NT + 3) / 4;            // k-steps over the 3 dy x 3 dx x 2 NT chunks
  static constexpr int UGA = 18 * NT - 4 * (KSA - 1);      // lane groups used in the last k-step
  static constexpr int WPART = NT * ((KSA - 1) * 1024 + UGA * 256);  // bytes of one packed weight part
  // operand prefetch distance (k-steps); the ring of PD + 1 register sets must
  // divide KSA so that m-tile i + 1's first steps land in the slots its loop reads
  static constexpr int PD = (KSA % 2 == 0) ? 1 : (KSA % 3 == 0) ? 2 : (KSA % 5 == 0) ? 4 : 0;
  static_assert(PD > 0 && KSA % (PD + 1) == 0, "operand ring");
  static constexpr int IMGB = 80 * 1024;                   // bytes per staging image (two: the whole LDS)
  static constexpr int PPW = (IMGB / 1024 + NW - 1) / NW;  // 1 KiB DMA pieces per wave per tile
  static constexpr int NGP = (PPW + 1) / 2;                // VGPRs of 16-bit staging offsets
  static constexpr int NTO = (KSA + 1) / 2;                // VGPRs of 16-bit tap offsets
  static constexpr int NRF = (NT + 1) / 2;                 // residual runs per pixel (16 B pairs, 8 B odd tile)
  static constexpr int NRL = SP * NRF;                     // residual loads per m-tile
  static constexpr int NS = SP * NRF;                      // stores per m-tile
  static constexpr int PRODUCTS = FM == 1 ? 3 : FM == 2 ? 2 : 1;
  // bf16x3 / f16x2 with a half-used last k-step (UGA = 2): its fragment holds the hi
  // weights in lane groups 0-1 and the lo weights of the same chunks in groups
  // 2-3, the activation offsets of groups 2-3 mirror 0-1, and two MFMAs (x hi,
  // x lo; f16x2: one, x) give all the products of those chunks (saves NT fragments)
  static constexpr bool MERGE = FM != 0 && UGA == 2;
  static constexpr int NPROD_LAST = MERGE ? (FM == 1 ? 2 : 1) : PRODUCTS;  // MFMAs per out-tile, last k-step
  // product T's weight part / activation part: bf16x3 (0,0) (0,1) (1,0); f16x2 (0,0) (1,0)
  static constexpr int wpart(int T) { return FM == 1 ? (T == 2 ? 1 : 0) : FM == 2 ? T : 0; }
  static constexpr int xpart(int T) { return FM == 1 && T == 1 ? 1 : 0; }
  // weight fragments held in the accumulator file: the first 64 (256 AGPRs)
  static constexpr bool in_agpr(int pt, int s, int n) { return (pt * KSA + s) * NT + n < 64; }
  // deferred-epilogue schedule, in epilogue steps (one k-step each): step n
  // finishes out-tile n; store i (pairs first, then the odd tile; hi then lo)
  // goes out on its own step once its tiles are done
  static constexpr int NPS = (NT / 2) * SP;  // pair stores
  static constexpr int store_tile(int i) { return i < NPS ? 2 * (i / SP) + 1 : NT - 1; }
  static constexpr int store_step(int i) {
    int st = -1;
    for (int k = 0; k <= i; ++k) st = store_tile(k) > st + 1 ? store_tile(k) : st + 1;
    return st;
  }
  // weight fragment offset (pack_block16_kernel layout): [part][k-step][n-tile][lane][8]
  static constexpr int xfrag(int part, int s, int n) {
    return part * WPART + (s < KSA - 1 ? (s * NT + n) * 1024 : (KSA - 1) * NT * 1024 + n * UGA * 256);
  }
};

// compile-time loop: f(KStep<0>{}) .. f(KStep<N-1>{})
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(KStep<I>{});
    static_for<N, I + 1>(f);
  }
}

// c (+)= w . x on v_mfma_f32_16x16x32_bf16 (ZC: c = w . x).  The weight
// fragments are pinned into the accumulator file where they were loaded (an
// empty asm with an "a" operand, G16W::in_agpr): without the pin hipcc keeps a
// builtin MFMA's A operand in VGPRs, spills 336 VGPRs of weights into AGPRs and
// copies them back before every MFMA; with it, the MFMA reads them in place.
// The MFMAs themselves stay builtins, so hipcc pads their hazards (an inline-asm
// MFMA chain lets hipcc insert accumulator copies it cannot see are hazards).
template <bool ZC, bool F16 = false>
__device__ __forceinline__ void mfma_w(f32x4& c, u32x4 w, u32x4 x) {
  if constexpr (F16)
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x),
                                               ZC ? f32x4{0.f, 0.f, 0.f, 0.f} : c, 0, 0, 0);
  else
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x),
                                                ZC ? f32x4{0.f, 0.f, 0.f, 0.f} : c, 0, 0, 0);
}

// ReLU of an accumulator: relu_keepnan (common.h), as torch.relu for every input,
// a NaN of either sign included.  (Rounds 2-3 used one integer max on the bits,
// which zeroes a -NaN; the compare + select costs one VALU more per value.)
__device__ __forceinline__ float relu_acc(float x) { return relu_keepnan(x); }

// host mirror: pixels one staging image may hold
static constexpr int g16w_img_px(int NT, int SP) { return 80 * 1024 / (32 * NT * SP); }

struct Block16WArgs {
  const __bf16* in;   // [n][H][W][CP*SP] pre-BN input; its BN is folded into wfrag/bias
  const __bf16* res;  // residual (pre-BN) or nullptr
  __bf16* out;        // pre-BN output, or nullptr (last layer)
  const char* wfrag;  // packed weight fragments (G16W::xfrag)
  float* chsum;       // last layer: [ntiles][NW][CP] channel sums, else nullptr
  int H, W, dil, lgd, TH, ntiles;  // dil = 1 << lgd
  int rem, nb1, nb0, nbc;          // band geometry (BandGeo) for TH
  LiveRef live;  // bf16x3 (FM 1) only, count may be null: the clips that run, of the launch's ntiles / nbc
};

template <int NT, int SP, bool LAST, bool RES, int FM = (SP == 2 ? 1 : 0)>
__global__ __launch_bounds__(256, 1) void block16w_kernel(Block16WArgs a) {
  using G = G16W<NT, SP, FM>;
  constexpr int KSA = G::KSA, PD = G::PD, CB = G::CB, CP = G::CP, NW = G::NW;
  __shared__ __attribute__((aligned(16))) char sa0[G::IMGB];
  __shared__ __attribute__((aligned(16))) char sa1[G::IMGB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const int i16 = lane & 15;

  const int GR = gridDim.x;
  const int bid = blockIdx.x;
  const int lb = ((GR & 7) == 0) ? (bid & 7) * (GR >> 3) + (bid >> 3) : bid;  // XCD-aware tile order
  int tile = lb;
  // (a device-held clip count -- FM 1, an ordered re-run round: the tiles of its first clips)
  int ntiles = a.ntiles;
  if constexpr (FM == 1) {
    if (a.live.count) ntiles = live_clips(a.live, a.ntiles / a.nbc) * a.nbc;
  }
  if (tile >= ntiles) return;  // whole workgroup, before any barrier

  // the layer's weight operand, resident for the whole launch
  u32x4 wr[G::WP][KSA][NT];
  {
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.wfrag, (short)0, G::WP * G::WPART, 0x00020000);
#pragma unroll
    for (int pt = 0; pt < G::WP; ++pt)
#pragma unroll
      for (int s = 0; s < KSA; ++s)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const bool used = s < KSA - 1 || g < G::UGA;
          int voff = used ? lane * 16 : 0x40000000, soff = G::xfrag(pt, s, n);
          if (G::MERGE && s == KSA - 1 && pt == 0 && !used) {  // lo weights of chunks g - 2
            voff = (lane - 16 * G::UGA) * 16;
            soff = G::xfrag(1, s, n);
          }
          wr[pt][s][n] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, voff, soff, 0));
          if (G::in_agpr(pt, s, n)) asm volatile("" : "+a"(wr[pt][s][n]));
        }
  }

  const int H = a.H, W = a.W, d = a.dil, lgd = a.lgd, TH = a.TH;
  const int RW = W + d;               // image pixels per row: W columns + one separator per column class
  const int RB = W * CB;              // bytes of one map row in HBM
  const int npx = (TH + 2) * RW + 1;  // image pixels (trailing separator)
  const int chunks = max(npx * CB / 16, 64);
  const int qd = W >> lgd, rd = W & (d - 1);  // column classes: rd of qd + 1 columns, d - rd of qd
  // image column of map column w (class c = w mod d, index k = w / d)
  auto img_col = [&](int w) {
    const int c = w & (d - 1);
    return 1 + c * (qd + 1) + (c < rd ? c : rd) + (w >> lgd);
  };

  // per k-step: the lane's A-fragment offset relative to its output pixel in the
  // image (chunk c = 4 s + g -> tap (dy, dx), channel chunk cc); 0 for the unused
  // lane groups of the last k-step (their weights are zero)
  // (16-bit pairs: |offset| < 2^15, checked on the host)
  unsigned toff2[G::NTO];
#pragma unroll
  for (int i = 0; i < G::NTO; ++i) toff2[i] = 0;
#pragma unroll
  for (int s = 0; s < KSA; ++s) {
    const int gg = (G::MERGE && s == KSA - 1 && g >= G::UGA) ? g - G::UGA : g;  // merged step: mirror
    const int c = 4 * s + gg;
    const int dy = c / (6 * NT), c6 = c - dy * (6 * NT);
    const int dx = c6 / (2 * NT), cc = c6 - dx * (2 * NT);
    const int t = (c < 18 * NT) ? ((dy - 1) * RW + (dx - 1)) * CB + cc * 16 : 0;
    toff2[s >> 1] |= ((unsigned)t & 0xffffu) << (16 * (s & 1));
  }
  auto toff = [&](int s) {  // sign-extended 16-bit field
    return (int)(toff2[s >> 1] << (16 * (1 - (s & 1)))) >> 16;
  };

  // staging: piece i of this wave covers 16-B chunks [st, st + 64) of the image
  // (st clamped so the last piece ends at the image end; surplus pieces repeat
  // it); the lane's chunk sits at byte gp relative to the band's first row in
  // its clip, stored as the 16-bit (gp + d RB) / 16; 0xffff (separator / past the
  // image) lands past the clip (host-checked), where the bounds check reads 0
  unsigned gp2[G::NGP];
#pragma unroll
  for (int i = 0; i < G::NGP; ++i) gp2[i] = 0;
#pragma unroll
  for (int i = 0; i < G::PPW; ++i) {
    const int st = min((wave + i * NW) * 64, chunks - 64);
    const int c = st + lane;
    const int P = c / (CB / 16);
    const int within = (c - P * (CB / 16)) * 16;
    const int slot = P / RW, col = P - slot * RW;
    // inverse of img_col: classes c < rd span qd + 2 image pixels, the rest qd + 1
    int cls, k;
    const int big = rd * (qd + 2);
    if (col < big) {
      cls = col / (qd + 2);
      k = col - cls * (qd + 2) - 1;
    } else {
      const int u = col - big;
      const int cu = u / (qd + 1);
      k = u - cu * (qd + 1) - 1;
      cls = rd + cu;
    }
    const bool ok = P < npx && k >= 0 && cls < d;
    const unsigned v = ok ? (unsigned)(slot * d * RB + (cls + (k << lgd)) * CB + within) / 16u : 0xffffu;
    gp2[i >> 1] |= v << (16 * (i & 1));
  }

  const int clip_bytes = H * RB;
  auto clip_rsrc = [&](const void* t, int b, bool ok) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)(ok ? t : (const void*)a.in) + (size_t)b * clip_bytes),
                                             (short)0, ok ? clip_bytes : 0, 0x00020000);
  };
  // tile -> clip, first row h0, valid class rows (wave-uniform scalar arithmetic)
  auto tile_geo = [&](int tt, int& b, int& h0, int& rows) {
    b = __builtin_amdgcn_readfirstlane(tt / a.nbc);
    const int bi = tt - b * a.nbc;
    int r, k, n;
    if (bi < a.rem * a.nb1) {
      r = bi / a.nb1;
      k = bi - r * a.nb1;
      n = (H >> lgd) + 1;
    } else {
      const int bj = bi - a.rem * a.nb1;
      const int rr = bj / a.nb0;
      k = bj - rr * a.nb0;
      r = a.rem + rr;
      n = H >> lgd;
    }
    h0 = __builtin_amdgcn_readfirstlane(r + ((k * TH) << lgd));
    rows = __builtin_amdgcn_readfirstlane(TH < n - k * TH ? TH : n - k * TH);
  };
  struct Src {
    __amdgpu_buffer_rsrc_t rs;
    int rowoff;  // (h0 - d) * RB: byte offset of image row slot 0
  };
  auto tile_src = [&](int tt) {
    const bool valid = tt < ntiles;
    int b = 0, h0 = 0, rows = 0;
    if (valid) tile_geo(tt, b, h0, rows);
    return Src{clip_rsrc(a.in, b, valid), (h0 - d) * RB};
  };
  auto issue_piece = [&](char* dst, const Src& src, int i) {
    const int st0 = (wave + i * NW) * 64;
    const int st = __builtin_amdgcn_readfirstlane(st0 < chunks - 64 ? st0 : chunks - 64);
    const unsigned v = (gp2[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    const __amdgpu_buffer_rsrc_t rs = src.rs;  // (a member operand makes the host pass drop the kernel stub)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + st * 16), 16,
                                             (unsigned)src.rowoff + v * 16u, 0, 0, 0);
  };

  // m-tile walk: the wave's it-th m-tile of a tile is pixel p = 16 (wave + 4 it) +
  // i16 = (row j, column w) of the band; stepping by 64 pixels moves (j, w) by
  // (64 / W, 64 % W) with a carry
  const int p0 = 16 * wave + i16;
  const int j0 = p0 / W, w0 = p0 - j0 * W;
  const int sj = 64 / W, sw = 64 - sj * W;
  struct MPos {
    int p, j, w;
  };
  auto mstep = [&](MPos m) {
    m.p += 64;
    m.w += sw;
    m.j += sj;
    if (m.w >= W) {
      m.w -= W;
      m.j += 1;
    }
    return m;
  };
  // image offset of the lane's pixel; pixels past the band's valid rows read a safe one
  auto mbase = [&](const MPos& m, int tpv) {
    return m.p < tpv ? ((m.j + 1) * RW + img_col(m.w)) * CB : (RW + 1) * CB;
  };

  // operand ring: slot S % (PD + 1) holds the A fragments (SP parts) of k-step S
  u32x4 oa[PD + 1][SP];
  auto load_a = [&](const char* img, int base, int s, u32x4 (&o)[SP]) {
#pragma unroll
    for (int pt = 0; pt < SP; ++pt) o[pt] = *(const u32x4*)(img + base + toff(s) + pt * CP * 2);
  };

  // deferred-epilogue state of the pending (previous) m-tile
  f32x4 accp[NT];
  uint4 rv[G::NRF][SP];  // its residual runs
  // EARLY (residual layers that store): an m-tile loads its own residual runs at
  // k-step 0 into rvn (copied to rv when it becomes the pending m-tile), so the
  // epilogue never waits behind the stores issued after them (vmcnt is in order)
  constexpr bool EARLY = RES && !LAST;
  uint4 rvn[G::NRF][SP];
  int pop = 0x40000000;  // its output offset in the clip (0x40000000: none)
  int tprev = -1;        // LAST: tile whose channel sums are being accumulated
  bool plast = false;    // LAST: the pending m-tile is the wave's last of its tile
  f32x4 csum[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    accp[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    csum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int f = 0; f < G::NRF; ++f)
#pragma unroll
    for (int pt = 0; pt < SP; ++pt) {
      rv[f][pt] = uint4{0u, 0u, 0u, 0u};
      rvn[f][pt] = uint4{0u, 0u, 0u, 0u};
    }
  __amdgpu_buffer_rsrc_t out_p = clip_rsrc(nullptr, 0, false);  // pending m-tile's clip (stores)

  // epilogue of the pending m-tile, one step per k-step: step n applies ReLU and
  // the residual to out-tile n and splits it into bf16 (hi, lo) (or, last
  // layer, adds it to the channel sums, flushed once per tile and wave); the
  // stores follow as their data is ready, one per step (G16W::store_step)
  constexpr int NSTO = LAST ? 0 : G::NS;
  constexpr int ELAST = NSTO ? G::store_step(NSTO - 1) : NT - 1;  // last epilogue step
  typename ActT<FM>::V4 h[SP][NT];
  auto epi_step = [&](auto ec) {
    constexpr int E = decltype(ec)::value;
    if constexpr (E < NT) {
      constexpr int n = E;
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = relu_acc(accp[n][k]);
      if constexpr (RES) {
        // tile n's 4 channels: elements (n & 1) * 4 .. +3 of its pair's run, or the odd tile's 8-B run
        constexpr int f = n >> 1, e0 = (n < (NT & ~1)) ? (n & 1) * 4 : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = e0 + k;
          // (the parts summed from the first: a 0.f start costs an add of +0 per value)
          float r = act_dec<FM>(rv[f][0][e >> 1], e);
          if constexpr (SP == 2) r += act_dec<FM>(rv[f][1][e >> 1], e);
          v[k] += r;
        }
      }
      if constexpr (LAST) {
        const bool valid = pop != 0x40000000;
#pragma unroll
        for (int k = 0; k < 4; ++k) csum[n][k] += valid ? v[k] : 0.f;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          h[0][n][k] = (typename ActT<FM>::T)v[k];
          if constexpr (SP == 2) h[SP - 1][n][k] = (__bf16)(v[k] - (float)h[0][n][k]);
        }
      }
    }
    if constexpr (LAST && E == NT - 1) {
      if (plast) {
        const __amdgpu_buffer_rsrc_t cs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.chsum + ((size_t)(tprev < 0 ? 0 : tprev) * NW + wave) * CP), (short)0, tprev < 0 ? 0 : CP * 4,
            0x00020000);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          f32x4 c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            c[k] = sum16_dpp(csum[n][k]);
          }
          const int co = (i16 == 0) ? co16(NT, n, 4 * g) * 4 : 0x40000000;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, c), cs, co, 0, 0);
          csum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    if constexpr (!LAST) {
      static_for<NSTO>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        if constexpr (G::store_step(I) == E) {
          if constexpr (I < G::NPS) {
            constexpr int pr = I / SP, pt = I % SP;
            const u32x2 lo = __builtin_bit_cast(u32x2, h[pt][2 * pr]), hi = __builtin_bit_cast(u32x2, h[pt][2 * pr + 1]);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{lo[0], lo[1], hi[0], hi[1]}, out_p, pop + 16 * g,
                                                   64 * pr + pt * CP * 2, 0);
          } else {
            constexpr int pt = I - G::NPS;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h[pt][NT - 1]), out_p, pop + 8 * g,
                                                  64 * (NT / 2) + pt * CP * 2, 0);
          }
        }
      });
    }
  };

  // residual runs of an m-tile (pairs: 16 B at 64 f + 16 g; odd tile: 8 B at 64 (NT/2) + 8 g)
  auto res_loads = [&](uint4 (&dst)[G::NRF][SP], __amdgpu_buffer_rsrc_t rr, int po) {
#pragma unroll
    for (int f = 0; f < G::NRF; ++f)
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) {
        if (f < NT / 2) {
          dst[f][pt] = __builtin_bit_cast(
              uint4, __builtin_amdgcn_raw_buffer_load_b128(rr, po + 16 * g, 64 * f + pt * CP * 2, 0));
        } else {
          const u32x2 t = __builtin_bit_cast(
              u32x2, __builtin_amdgcn_raw_buffer_load_b64(rr, po + 8 * g, 64 * f + pt * CP * 2, 0));
          dst[f][pt] = uint4{t[0], t[1], 0u, 0u};
        }
      }
  };

  // k-steps: staging pieces of the next tile (first m-tile) on 1 .. KE - 1, the
  // pending epilogue on KE .. KE + ELAST, this m-tile's residual loads after it
  constexpr int KE = (KSA - ELAST - 2 >= 2) ? KSA - ELAST - 2 : 2;
  constexpr int KR = (KE + ELAST + 1 < KSA) ? KE + ELAST + 1 : KSA - 1;
  // VMEM ops a wave issues after its last staging piece of a tile, at least:
  // the pending m-tile's stores (and, late residual loads, this m-tile's)
  constexpr int NTOP = NSTO + (RES && !EARLY ? G::NRL : 0);

  // One m-tile: KSA k-steps of PRODUCTS x NT MFMAs; the operands of step S + PD
  // (or of the next m-tile's first steps, at image offset bnext) load under step
  // S's MFMAs.  FIRST: the wave's first m-tile of the tile, which also issues
  // the next tile's staging pieces (k-steps 1 .. KE - 1).  At k-step KE: the
  // pending m-tile's epilogue (after its residual runs landed: only this
  // m-tile's staging pieces are younger), then this m-tile's residual loads.
  auto run_mtile = [&](auto firstc, const char* img, char* nxt, const Src& sn, int bcur, int bnext,
                       __amdgpu_buffer_rsrc_t rr, int po, f32x4 (&acc)[NT]) {
    constexpr bool FIRST = decltype(firstc)::value;
    static_for<KSA>([&](auto sc) {
      constexpr int S = decltype(sc)::value;
      constexpr int SN = S + PD;
      if constexpr (EARLY && S == 0) res_loads(rvn, rr, po);  // before this m-tile's staging pieces
      if constexpr (SN < KSA) load_a(img, bcur, SN, oa[SN % (PD + 1)]);
      else load_a(img, bnext, SN - KSA, oa[SN % (PD + 1)]);
      // the operand reads go out ahead of this step's MFMAs (left to itself the
      // scheduler sinks them below most of the step and then waits on them)
      __builtin_amdgcn_sched_barrier(0);
      const u32x4 (&ac)[SP] = oa[S % (PD + 1)];
      constexpr int NPROD = S == KSA - 1 ? G::NPROD_LAST : G::PRODUCTS;
      static_for<NPROD>([&](auto tc) {
        constexpr int T = decltype(tc)::value;
        constexpr int WP = G::wpart(T), XP = G::xpart(T);
        static_for<NT>([&](auto nc) {
          constexpr int N = decltype(nc)::value;
          mfma_w<S == 0 && T == 0, FM == 2>(acc[N], wr[WP][S][N], ac[XP]);
        });
      });
      if constexpr (FIRST && S >= 1 && S < KE) {
        constexpr int NSTEP = KE - 1;  // k-steps carrying staging pieces
#pragma unroll
        for (int i = 0; i < G::PPW; ++i)
          if ((i * NSTEP) / G::PPW == S - 1) issue_piece(nxt, sn, i);
      }
      // res(pending) landed: only this m-tile's staging pieces are younger
      if constexpr (RES && !EARLY && S == KE) wait_vmcnt<(FIRST ? G::PPW : 0)>();
      static_for<ELAST + 1>([&](auto ec) {
        constexpr int E = decltype(ec)::value;
        if constexpr ((KE + E < KSA ? KE + E : KSA - 1) == S) epi_step(ec);
      });
      if constexpr (RES && !EARLY && S == KR) res_loads(rv, rr, po);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // prologue: DMA(first tile) -> sa0, then NTOP stand-in stores so the first
  // barrier sees the steady-state vmcnt layout
  {
    const Src s0 = tile_src(tile);
#pragma unroll
    for (int i = 0; i < G::PPW; ++i) issue_piece(sa0, s0, i);
  }
  {
    const __amdgpu_buffer_rsrc_t nul = clip_rsrc(nullptr, 0, false);
#pragma unroll
    for (int i = 0; i < NTOP; ++i) __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, nul, 0, i * 8, 0);
  }

  auto run_tile = [&](const char* cur, char* nxt) {
    int b, h0, rows;
    tile_geo(tile, b, h0, rows);
    const int tpv = rows * W;
    const int nmt = (tpv + 15) >> 4;
    const int nw_mt = (nmt - wave + NW - 1) / NW;  // this wave's m-tiles (at least one: a dummy)
    const int niter = __builtin_amdgcn_readfirstlane(nw_mt > 1 ? nw_mt : 1);
    const int tnext = tile + GR;
    const int rowoff = h0 * RB, dRB = d * RB;

    // DMA(tile) landed (this wave's pieces: NTOP ops are younger) ...
    wait_vmcnt<NTOP>();
    __builtin_amdgcn_s_barrier();  // ... and every wave's; every wave is done with `nxt`
    const Src sn = tile_src(tnext);
    const __amdgpu_buffer_rsrc_t rr = clip_rsrc(a.res, b, RES);
    const __amdgpu_buffer_rsrc_t outr = clip_rsrc(a.out, b, !LAST);

    MPos m{p0, j0, w0};
    int bcur = mbase(m, tpv);
#pragma unroll
    for (int s = 0; s < PD; ++s) load_a(cur, bcur, s, oa[s]);
    for (int it = 0; it < niter; ++it) {
      const bool more = it + 1 < niter;
      const MPos mn = mstep(m);
      const int bnext = more ? mbase(mn, tpv) : bcur;
      // this m-tile's output offset (the folded-BN bias rides in input channel C)
      const int po = m.p < tpv ? rowoff + m.j * dRB + m.w * CB : 0x40000000;
      f32x4 acc[NT];
      if (it == 0)
        run_mtile(std::integral_constant<bool, true>{}, cur, nxt, sn, bcur, bnext, rr, po, acc);
      else
        run_mtile(std::integral_constant<bool, false>{}, cur, nxt, sn, bcur, bnext, rr, po, acc);
      // this m-tile becomes the pending epilogue
#pragma unroll
      for (int n = 0; n < NT; ++n) accp[n] = acc[n];
      pop = po;
      out_p = outr;
      if constexpr (EARLY) {
#pragma unroll
        for (int f = 0; f < G::NRF; ++f)
#pragma unroll
          for (int pt = 0; pt < SP; ++pt) rv[f][pt] = rvn[f][pt];
      }
      tprev = tile;
      plast = !more;
      m = mn;
      bcur = bnext;
    }
    tile = tnext;
  };

  while (true) {
    run_tile(sa0, sa1);
    if (tile >= ntiles) break;
    run_tile(sa1, sa0);
    if (tile >= ntiles) break;
  }
  wait_vmcnt<0>();
  static_for<ELAST + 1>([&](auto ec) { epi_step(ec); });
}
