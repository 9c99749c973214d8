// ---------------------------------------------------------------------------- //
// Split band kernel (block16s_kernel): one res block layer of the 16-bit formats for
// the latency schedule -- chunks of fewer clips than CUs, where a schedule of whole
// clips per workgroup (the fused pairs, block16l_kernel) leaves all but `clips` CUs idle.
//
// A workgroup computes ONE tile and leaves: tile = (clip, dilation class, band of TH
// class rows, out-tile n).  Geometry, staging image and packed fragments are
// block16w_kernel's (res_bf16w.inc): the image of rows + 2 class rows in column-class
// order with zero separators, the lane's tap offsets, co16's channel runs.  What differs
// is the weight operand.  block16w_kernel is built to amortise: each of its four waves
// first loads the layer's whole operand (WP x KSA x NT fragments, 336 VGPRs at bf16x3),
// which at one to three m-tiles per workgroup IS the launch.  Here the out-tiles (16
// channels) are dealt to workgroups: a wave holds the WP x KSA fragments of its out-tile
// only (112 VGPRs at bf16x3, a third of the operand; the 4 waves of a workgroup and the
// NT workgroups of a band read them from L2), and the map gets NT times the workgroups.
// (Fetching fragments per k-step from LDS, as block16r_kernel, would have every
// workgroup copy the whole operand into its LDS first: the same prologue in another place.)
//
// Per output the arithmetic is block16w_kernel's, instruction for instruction: the
// k-steps in order, per k-step the products in order (G16W::wpart / xpart, the merged
// last step), ReLU, the residual parts summed then added, RNE / the (hi, lo) split -- so a
// stored layer is bit-for-bit the weight-stationary layer's (and the fused pair's).
// The last layer (VOUT) does not sum: it writes relu(y) (+ residual) in fp32 per pixel,
// and chsum_stream_kernel / chsum_band_kernel (below) add those values in exactly the
// order block16l_kernel / block16w_kernel would have, into the same partials.
// No workgroup waits on another; a launch is one layer.
//
// ROWB: the same tiles with block16r_kernel's arithmetic (res_bf16r.inc), for the models the
// throughput schedule runs on the row-band kernel.  That kernel reads the same packed
// fragments and the same activations (its conv0 leaves the bias channel 0), but per output it
// starts the accumulator at the folded-BN bias of the pixel's border class (the table
// pack_bias16_kernel wrote), runs all the products in the last k-step too (no merged step: the
// unused lane groups multiply zero weights by a zero pixel), and adds the residual as one
// selection-matrix MFMA per part (hi, then lo).  ROWB does exactly that, so its stored layers
// are block16r_kernel's bit for bit; chsum_rowband_kernel rebuilds its per-m-tile partials.
// ---------------------------------------------------------------------------- //
struct Block16SArgs {
  const __bf16* in;   // [n][H][W][CP*SP] pre-BN input
  const __bf16* res;  // residual (pre-BN) or nullptr
  __bf16* out;        // pre-BN output (VOUT: unused)
  const char* wfrag;  // packed weight fragments (G16W::xfrag)
  float* vout;        // VOUT: [n][H][W][CP] fp32 relu(y) (+ residual), map order
  const float* bias;  // ROWB: [16][CP] folded input-BN shift per border class
  int H, W, dil, lgd, TH, nclips;
  int rem, nb1, nb0, nbc;  // band geometry (BandGeo) for TH
  LiveRef live;            // count may be null: the clips that run, of the launch's nclips
};

template <int NT, int SP, bool VOUT, bool RES, int FM, bool ROWB = false>
__global__ __launch_bounds__(256, 2) void block16s_kernel(Block16SArgs a) {
  static_assert(!ROWB || FM != 2, "the row-band family has no f16x2");
  using G = G16W<NT, SP, FM>;
  constexpr bool MERGE = G::MERGE && !ROWB;
  constexpr int KSA = G::KSA, CB = G::CB, CP = G::CP, NW = G::NW;
  __shared__ __attribute__((aligned(16))) char img[G::IMGB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const int i16 = lane & 15;

  // blockIdx -> (band tile, out-tile): the NT workgroups of a band are neighbours
  const int tile = (int)blockIdx.x / NT;
  const int n = (int)blockIdx.x - tile * NT;
  const int b = tile / a.nbc;
  if (a.live.count && b >= live_clips(a.live, a.nclips)) return;  // whole workgroup, before any barrier

  const int H = a.H, W = a.W, d = a.dil, lgd = a.lgd, TH = a.TH;
  const int RW = W + d;   // image pixels per row: W columns + one separator per column class
  const int RB = W * CB;  // bytes of one map row in HBM
  const int qd = W >> lgd, rd = W & (d - 1);
  auto img_col = [&](int w) {
    const int c = w & (d - 1);
    return 1 + c * (qd + 1) + (c < rd ? c : rd) + (w >> lgd);
  };

  // the tile's band: class r, first row h0, valid class rows (block16w_kernel's tile_geo)
  int h0, rows;
  {
    const int bi = tile - b * a.nbc;
    int r, k, nr;
    if (bi < a.rem * a.nb1) {
      r = bi / a.nb1;
      k = bi - r * a.nb1;
      nr = (H >> lgd) + 1;
    } else {
      const int bj = bi - a.rem * a.nb1;
      const int rr = bj / a.nb0;
      k = bj - rr * a.nb0;
      r = a.rem + rr;
      nr = H >> lgd;
    }
    h0 = r + ((k * TH) << lgd);
    rows = TH < nr - k * TH ? TH : nr - k * TH;
  }
  const int clip_bytes = H * RB;
  auto clip_rsrc = [&](const void* t, bool ok) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)(ok ? t : (const void*)a.in) + (size_t)b * clip_bytes),
                                             (short)0, ok ? clip_bytes : 0, 0x00020000);
  };

  // staging: the image of rows + 2 class rows, 1 KiB pieces dealt to the waves; a chunk
  // that is a separator, past the image or on a row outside the map gets an offset past
  // the clip, where the bounds check reads 0 (the last piece is clamped to the image's end)
  {
    const int npx = (rows + 2) * RW + 1;
    const int chunks = max(npx * CB / 16, 64);
    const __amdgpu_buffer_rsrc_t rs = clip_rsrc(a.in, true);
    const unsigned rowoff = (unsigned)((h0 - d) * RB);  // image row slot 0 (may lie above the map)
    const int big = rd * (qd + 2);
    for (int st0 = wave * 64; st0 < chunks; st0 += NW * 64) {
      const int st = __builtin_amdgcn_readfirstlane(st0 < chunks - 64 ? st0 : chunks - 64);
      const int c = st + lane;
      const int P = c / (CB / 16);
      const int within = (c - P * (CB / 16)) * 16;
      const int slot = P / RW, col = P - slot * RW;
      int cls, k;  // inverse of img_col: classes c < rd span qd + 2 image pixels, the rest qd + 1
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
      const unsigned voff = ok ? rowoff + (unsigned)(slot * d * RB + (cls + (k << lgd)) * CB + within) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + st * 16), 16, voff,
                                               0, 0, 0);
    }
  }

  // the out-tile's weight fragments (loads in flight with the staging)
  u32x4 wr[G::WP][KSA];
  {
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.wfrag, (short)0, G::WP * G::WPART, 0x00020000);
#pragma unroll
    for (int pt = 0; pt < G::WP; ++pt)
#pragma unroll
      for (int s = 0; s < KSA; ++s) {
        const bool used = s < KSA - 1 || g < G::UGA;
        int voff = used ? lane * 16 : 0x40000000, soff = G::xfrag(pt, s, n);
        if (MERGE && s == KSA - 1 && pt == 0 && !used) {  // lo weights of chunks g - 2
          voff = (lane - 16 * G::UGA) * 16;
          soff = G::xfrag(1, s, n);
        }
        wr[pt][s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, voff, soff, 0));
      }
  }

  // per k-step: the lane's A-fragment offset relative to its output pixel in the image
  int toff[KSA];
#pragma unroll
  for (int s = 0; s < KSA; ++s) {
    const int gg = (MERGE && s == KSA - 1 && g >= G::UGA) ? g - G::UGA : g;  // merged step: mirror
    const int c = 4 * s + gg;
    const int dy = c / (6 * NT), c6 = c - dy * (6 * NT);
    const int dx = c6 / (2 * NT), cc = c6 - dx * (2 * NT);
    toff[s] = (c < 18 * NT) ? ((dy - 1) * RW + (dx - 1)) * CB + cc * 16 : 0;
  }

  const int tpv = rows * W;
  const int nmt = (tpv + 15) >> 4;
  const int niter = __builtin_amdgcn_readfirstlane((nmt - wave + NW - 1) / NW);  // this wave's m-tiles (may be 0)
  const int cob = co16(NT, n, 4 * g) * 2;  // the lane's 4-channel run of out-tile n, bytes within a part
  const __amdgpu_buffer_rsrc_t rr = clip_rsrc(a.res, RES);
  const __amdgpu_buffer_rsrc_t outr = clip_rsrc(a.out, !VOUT);

  // the image has landed: this wave's pieces, then every wave's
  asm volatile("" ::: "memory");
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // MI m-tiles at a time: their MFMA chains (each its own accumulator, each in block16w_kernel's
  // order) interleave, so one m-tile's operand reads and MFMA latency hide under the other's
  constexpr int MI = 2;
  for (int it0 = 0; it0 < niter; it0 += MI) {
    bool pv[MI];
    int base[MI], po[MI], hw[MI];  // image offset, output offset in the clip, map pixel h * W + w
    u32x2 rv[MI][SP];
    u32x4 rvr[MI][SP];  // ROWB: the 16-B residual runs of the out-tile's pair (block16r_kernel's res_loads)
    f32x4 acc[MI];
#pragma unroll
    for (int u = 0; u < MI; ++u) {
      const int p = 16 * (wave + NW * (it0 + u)) + i16;
      pv[u] = it0 + u < niter && p < tpv;
      const int j = p / W, w = p - j * W;
      base[u] = pv[u] ? ((j + 1) * RW + img_col(w)) * CB : (RW + 1) * CB;  // past the band: a safe pixel
      po[u] = pv[u] ? (h0 + j * d) * RB + w * CB : 0x40000000;
      hw[u] = (h0 + j * d) * W + w;
      if constexpr (RES && !ROWB) {
#pragma unroll
        for (int pt = 0; pt < SP; ++pt)
          rv[u][pt] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rr, po[u] + cob, pt * CP * 2, 0));
      }
      if constexpr (RES && ROWB) {
        const int f = n >> 1;
        const int o = (f < NT / 2 || g < 2) ? po[u] + 16 * g : 0x40000000;
#pragma unroll
        for (int pt = 0; pt < SP; ++pt)
          rvr[u][pt] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, o, 64 * f + pt * CP * 2, 0));
      }
      if constexpr (ROWB) {  // the accumulator starts at the bias of the pixel's border class
        const int h = h0 + (pv[u] ? j : 0) * d, wc = pv[u] ? w : 0;
        const int cls = (wc < d ? 4 : 0) | (wc + d >= W ? 8 : 0) | (h < d ? 1 : 0) | (h + d >= H ? 2 : 0);
        acc[u] = *(const f32x4*)(a.bias + cls * CP + co16(NT, n, 4 * g));
      }
    }
    static_for<KSA>([&](auto sc) {
      constexpr int S = decltype(sc)::value;
      u32x4 x[MI][SP];
#pragma unroll
      for (int u = 0; u < MI; ++u)
#pragma unroll
        for (int pt = 0; pt < SP; ++pt) {
          int off = base[u] + toff[S] + pt * CP * 2;
          // ROWB: the last k-step's unused lane groups read zeros (the image's first pixel is a separator)
          if constexpr (ROWB && S == KSA - 1 && G::UGA < 4) off = g < G::UGA ? off : pt * CP * 2;
          x[u][pt] = *(const u32x4*)(img + off);
        }
      constexpr int NPROD = (S == KSA - 1 && !ROWB) ? G::NPROD_LAST : G::PRODUCTS;
      static_for<NPROD>([&](auto tc) {
        constexpr int T = decltype(tc)::value;
#pragma unroll
        for (int u = 0; u < MI; ++u)
          mfma_w<S == 0 && T == 0 && !ROWB, FM == 2>(acc[u], wr[G::wpart(T)][S], x[u][G::xpart(T)]);
      });
    });
    // epilogue of out-tile n (block16w_kernel's epi_step)
#pragma unroll
    for (int u = 0; u < MI; ++u) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = relu_acc(acc[u][k]);
      if constexpr (RES && ROWB) {
        // + residual as block16r_kernel adds it: a 0/1 selection matrix times the run, per part
        bf16x8 e;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
          e[jj] = (co16(NT, n, i16) == 32 * (n >> 1) + 8 * g + jj) ? (__bf16)1.0f : (__bf16)0.0f;
#pragma unroll
        for (int pt = 0; pt < SP; ++pt)
          v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(e, __builtin_bit_cast(bf16x8, rvr[u][pt]), v, 0, 0, 0);
      }
      if constexpr (RES && !ROWB) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float r = act_dec<FM>(rv[u][0][k >> 1], k);
          if constexpr (SP == 2) r += act_dec<FM>(rv[u][1][k >> 1], k);
          v[k] += r;
        }
      }
      if constexpr (VOUT) {
        if (pv[u]) *(f32x4*)(a.vout + ((size_t)b * H * W + hw[u]) * CP + co16(NT, n, 4 * g)) = v;
      } else {
        typename ActT<FM>::V4 h[SP];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          h[0][k] = (typename ActT<FM>::T)v[k];
          if constexpr (SP == 2) h[SP - 1][k] = (__bf16)(v[k] - (float)h[0][k]);
        }
#pragma unroll
        for (int pt = 0; pt < SP; ++pt)
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h[pt]), outr, po[u] + cob, pt * CP * 2, 0);
      }
    }
  }
}

// The channel-sum partials of the last layer from block16s_kernel's per-pixel values, added
// in the order of the kernel the throughput schedule runs there, so that tail_sum_kernel
// sees the same partials bit for bit.
//
// block16l_kernel's: [clip][2][CP].  Its wave widx = 0, 1 walks the clip's STREAM pixels q
// (rows in dilation-class order: class c's rows c, c + d, ..., the classes one after
// another; pixel q = stream row * W + column) 16 widx + i16 + 32 t, t = 0, 1, ..., adding
// each lane's values in that order, then the lane group's 16 lanes by sum16_dpp.
// One workgroup of two waves per clip; U pixels' loads in flight per lane.
template <int NT>
__global__ __launch_bounds__(128) void chsum_stream_kernel(const float* __restrict__ vout, float* __restrict__ chsum,
                                                           int H, int W, int d, int lgd, LiveRef live) {
  constexpr int CP = 16 * NT, U = NT == 3 ? 8 : 16;
  const int clip = blockIdx.x;
  if (live.count && clip >= live_clips(live, (int)gridDim.x)) return;
  const int lane = threadIdx.x & 63, widx = threadIdx.x >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int HW = H * W;
  const int qd = H >> lgd, q1 = qd + 1, rem = H - (qd << lgd);
  const float* v = vout + (size_t)clip * HW * CP;
  f32x4 cs[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) cs[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q0 = 16 * widx + i16; q0 - i16 < HW; q0 += 32 * U) {  // (q0 - i16: the loop count is the wave's)
    f32x4 t[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + 32 * u;
      const bool ok = q < HW;
      const int rl = ok ? q / W : 0, w = ok ? q - rl * W : 0;
      int c, j;  // stream row -> (class, class row)
      if (rl < rem * q1) {
        c = rl / q1;
        j = rl - c * q1;
      } else {
        const int tt = rl - rem * q1;
        const int cu = qd > 0 ? tt / qd : 0;
        c = rem + cu;
        j = tt - cu * qd;
      }
      const float* pv = v + ((size_t)(c + (j << lgd)) * W + w) * CP;
#pragma unroll
      for (int n = 0; n < NT; ++n)
        t[u][n] = ok ? *(const f32x4*)(pv + co16(NT, n, 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int n = 0; n < NT; ++n) cs[n] += t[u][n];
  }
  float* out = chsum + ((size_t)clip * 2 + widx) * CP;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    f32x4 c;
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = sum16_dpp(cs[n][k]);
    if (i16 == 0) *(f32x4*)(out + co16(NT, n, 4 * g)) = c;
  }
}

// block16w_kernel's: [tile][4][CP], tile = (clip, class, band of TH class rows) of ITS plan
// (TH, the band geometry: the arguments).  Wave `wave` of a tile adds its m-tiles wave,
// wave + 4, ... (16 band pixels each, lane i16's pixel p = 16 m + i16, band row p / W) in
// order, then sum16_dpp.  One workgroup of four waves per tile.
template <int NT>
__global__ __launch_bounds__(256) void chsum_band_kernel(const float* __restrict__ vout, float* __restrict__ chsum,
                                                         int H, int W, int d, int lgd, int TH, int rem, int nb1,
                                                         int nb0, int nbc, int nclips, LiveRef live) {
  constexpr int CP = 16 * NT, NW = 4;
  const int tile = blockIdx.x;
  const int b = tile / nbc;
  if (live.count && b >= live_clips(live, nclips)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int bi = tile - b * nbc;
  int r, k, nr;
  if (bi < rem * nb1) {
    r = bi / nb1;
    k = bi - r * nb1;
    nr = (H >> lgd) + 1;
  } else {
    const int bj = bi - rem * nb1;
    const int rr = bj / nb0;
    k = bj - rr * nb0;
    r = rem + rr;
    nr = H >> lgd;
  }
  const int h0 = r + ((k * TH) << lgd);
  const int rows = TH < nr - k * TH ? TH : nr - k * TH;
  const int tpv = rows * W;
  const float* v = vout + (size_t)b * H * W * CP;
  f32x4 cs[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) cs[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p = 16 * wave + i16; p - i16 < tpv; p += 16 * NW) {
    const bool ok = p < tpv;
    const int j = ok ? p / W : 0, w = ok ? p - j * W : 0;
    const float* pv = v + ((size_t)(h0 + j * d) * W + w) * CP;
#pragma unroll
    for (int n = 0; n < NT; ++n) cs[n] += ok ? *(const f32x4*)(pv + co16(NT, n, 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float* out = chsum + ((size_t)tile * NW + wave) * CP;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    f32x4 c;
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) c[k2] = sum16_dpp(cs[n][k2]);
    if (i16 == 0) *(f32x4*)(out + co16(NT, n, 4 * g)) = c;
  }
}

// block16r_kernel's: [tile][8 waves][MT m-tiles][CP], tile = a band of ITS plan (TH, MT, the band
// geometry: the arguments): one partial per m-tile, the 16 pixels p = 16 (wave MT + m) + i16
// of the band (row p / W; valid while inside the band's TH rows and the map) by sum16_dpp.
// One workgroup of four waves per tile, a wave per m-tile slot at a time.
template <int NT>
__global__ __launch_bounds__(256) void chsum_rowband_kernel(const float* __restrict__ vout, float* __restrict__ chsum,
                                                            int H, int W, int d, int TH, int MT, int rem, int nb1,
                                                            int nb0, int nbc, int nclips, LiveRef live) {
  constexpr int CP = 16 * NT;
  const int tile = blockIdx.x;
  const int b = tile / nbc;
  if (live.count && b >= live_clips(live, nclips)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int h0 = band_h0(tile - b * nbc, rem, nb1, nb0, TH, d);
  const float* v = vout + (size_t)b * H * W * CP;
  for (int slot = wave; slot < 8 * MT; slot += 4) {  // slot = wave' MT + m of block16r_kernel
    const int p = 16 * slot + i16;
    const int j = p / W, w = p - j * W, h = h0 + j * d;
    const bool ok = p < TH * W && h < H;
    const float* pv = v + ((size_t)(ok ? h : 0) * W + (ok ? w : 0)) * CP;
    float* out = chsum + ((size_t)tile * 8 * MT + slot) * CP;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const f32x4 t = ok ? *(const f32x4*)(pv + co16(NT, n, 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 c;
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = sum16_dpp(t[k]);
      if (i16 == 0) *(f32x4*)(out + co16(NT, n, 4 * g)) = c;
    }
  }
}
