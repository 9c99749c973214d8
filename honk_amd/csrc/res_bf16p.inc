// ---------------------------------------------------------------------------- //
// Fused res block pair (block16p_kernel): an odd layer A and the even layer B
// that follows it, in one launch, with A's output kept on chip.
//
// Why: the weight-stationary kernel (res_bf16w.inc) runs near the chip's memory
// throughput -- per pair of layers it moves 5.5 activation tensors (A: staged
// input with its halo rows, output; B: staged input, residual, output).  Here A's
// output never leaves the CU and the pair moves 3: A's input once (rows are
// streamed, each loaded exactly once), B's residual (the same tensor, re-read
// from L2/MALL) and B's output (written over it in place).
//
// Decomposition.  A's dilation d splits every clip's rows into d classes (rows
// c, c + d, c + 2d, ...); in class-row units A is a plain 3-row conv and B (at
// dilation d or 2d) a 3-row conv with taps sB = 1 or 2 class rows apart.  A
// workgroup owns whole clips and walks one STREAM: its clips' rows in (clip,
// class, class row) order, W pixels each.  Step k:
//   * waves 0, 1 (SIMDs 0, 1) compute A on stream pixels [kP, kP + P), reading
//     the A-in ring (rows streamed from HBM by LDS-DMA, one step ahead) and
//     writing the bf16 (hi, lo) result into the A-out ring;
//   * waves 2, 3 compute B on stream pixels [kP - lag - P, kP - lag), reading the
//     A-out ring, adding the residual from HBM and storing the layer's output;
//   * one s_barrier per step.
// Each wave keeps its layer's whole weight operand in the VGPR/AGPR file (as in
// block16w_kernel), so one SIMD pair runs A and the other B, concurrently.
// The lag (host-computed, plan_pair) keeps B behind the rows A has finished;
// the ring sizes keep a slot alive until its last reader is done.
//
// Zero padding without separators: every tap of every lane is checked against
// its class-row unit and the map columns once per m-tile (tap base tb[9]); an
// invalid tap points at a zeroed LDS block, so the MFMA loop has no predicates.
// The folded-BN border bias rides in the zero-padding channel C exactly as in
// block16w_kernel (1.0 at valid pixels, 0 in the zero block), so the pair
// computes bit-for-bit what the two single-layer launches compute.
// ---------------------------------------------------------------------------- //

// experiment switches (exp/pair_ab.sh builds variants): the prefetch distance one k-step
// short of the operand sets, the A epilogue's packed fp16 ReLU
#ifndef HONK_PAIR_PDM
#define HONK_PAIR_PDM 0
#endif
#ifndef HONK_PAIR_PKRELU
#define HONK_PAIR_PKRELU 1
#endif
#ifndef HONK_PAIR_MIX
#define HONK_PAIR_MIX 1
#endif
// DTOP: A's k-steps 0 and 1 of a step in one scheduling region with the head of the step's
// block (see run_mtile; 0: every k-step fenced, the head's scalar work ahead of the first
// MFMA, measured 1 % slower).  res_vf.hip, the unit that compiles the pair and last-layer
// kernels, turns it on.
#ifndef HONK_PAIR_DTOP
#define HONK_PAIR_DTOP 0
#endif

struct Block16PArgs {
  __bf16* R;            // [n][H][W][CP*SP] pre-BN x_{i-1}: A's input and B's residual; B's output in place
  const char* wA;       // A's packed weight fragments (G16W::xfrag layout)
  const char* wB;       // B's
  unsigned chunk_bytes;  // n * H * W * CB (the buffer range; < 0xF0000000)
  int nclips, H, W;
  int d, lgd, sB;       // A's dilation (= 1 << lgd) and B's tap stride in class rows (1 or 2)
  int lag;              // B's lag behind A in stream pixels
  int NRA, NRB;         // ring slots (A input, A output)
  int slotb;            // bytes per ring slot (>= ppr KiB, = W * PXB mod 256)
  int ppr;              // 1 KiB DMA pieces per row
  float* chsum;         // last-layer mode: [nclips][2][CP] channel sums of relu(A's output)
  int padb;             // PADC: bytes of zero columns left of a slot's row (and at least as many right)
  int ringpad;          // PADC, shared pads: a slot's right pad is the next slot's left pad (ring A's
                        // last slot's: ring B's first), ring B carries one more pad past its last slot
                        // (0: every slot has both pads)
  LiveRef live;         // bf16x3 (FM 1) only, count may be null: the clips that run, of the launch's nclips
};

template <int NT, int SP>
struct G16P {
  static constexpr int P = 64;    // stream pixels per layer per step: 2 m-tiles per wave
  static constexpr int ZB = 256;  // zero block bytes
  // LDS pixel pitch: the CB-byte pixel padded to 16 B x (2 mod 4).  A b128 lane
  // group reads chunk c for 8 pixels (lanes 0-3, 12-15 of group g) and chunk c + 1
  // for the 8 others (lanes 4-11 of group g + 1): 16 consecutive pixels at a pitch
  // of 2 mod 4 quad-banks land on the 8 even quad-banks, each once, per half, so
  // chunk c (even offset) and c + 1 (odd) fill all 16 -- conflict-free.  (An odd
  // pitch, e.g. the unpadded 12 or 13, always leaves a 2-way conflict.)
  static constexpr int PXB = 16 * ((G16W<NT, SP>::CB / 16 + 1) / 4 * 4 + 2);
};
// host mirror of G16P::PXB
static constexpr int g16p_pxb(int NT, int SP) { return 16 * ((32 * NT * SP / 16 + 1) / 4 * 4 + 2); }

// host mirror
static constexpr int g16p_lds_bytes() { return 160 * 1024; }
// f16x2's row-entry tables (block16p_body TBL): the zero block every invalid tap
// reads from its start (an m-tile's k-steps reach 64 (KSA - 1) + 64 bytes past a
// tap's base), and per wave TR entries of TEB bytes
static constexpr int g16p_zb_tbl() { return 1024; }
static constexpr int g16p_tr() { return 32; }
static constexpr int g16p_teb() { return 32; }
// LDS past the rings: zero block, the 1 KiB sink, [TBL: the waves' tables and a
// zeroed slot, the tap rows of rows outside their class]
static constexpr int g16p_lds_extra(bool tbl, int wps, int slotb) {
  return tbl ? g16p_zb_tbl() + 1024 + wps * g16p_tr() * g16p_teb() + slotb : 256 + 1024;
}
// Two streams on the row table (block16p_body SHZ): the zero block, the sink and the zeroed
// slot are read-only zeros / a write-only sink, so the streams share one copy at the start
// of the LDS (256-B rounded); each stream's share past it holds its rings and its waves'
// tables.  (res8's 13-pixel rows need 16 + 17 ring slots per stream: with a copy per stream
// they missed half the LDS by 1.5 KiB.)  The zeroed slot (zb: a slot and, with shared pads, the
// extra pad its last row reads) starts the LDS and doubles as the zero block; the sink follows.
static constexpr int g16p_sink_off(int zb) { return ((zb > g16p_zb_tbl() ? zb : g16p_zb_tbl()) + 255) / 256 * 256; }
static constexpr int g16p_shared_bytes(int zb) { return g16p_sink_off(zb) + 1024; }
static constexpr int g16p_stream_bytes(int ns, int slotb) {
  return ((g16p_lds_bytes() - g16p_shared_bytes(slotb)) / ns) / 256 * 256;
}

// NS streams per workgroup (NS = 2: the bf16 mode, whose rings fit half the LDS):
// waves 4 s .. 4 s + 3 run stream s on its own half of the LDS and its own half of
// the workgroup's clips, so every SIMD holds one wave of each stream and the matrix
// pipe is fed by one while the other issues its VALU / memory work.  Both streams
// take the same number of steps (the longer one's): the step barrier is common.
//
// LM (last-layer mode, block16l_kernel): the model's last layer when it is odd (no
// residual, res15's layer 13) on the same machinery with layer A only: every stream
// is 2 A waves (NS = 2: one wave per SIMD), no
// A-out ring, and instead of an output the epilogue sums relu(A) per channel.  A
// stream runs its clips one at a time (the walk restarts at each clip), so a
// lane's pixels of a clip -- and the order of its sums -- do not depend on the
// clip's position in the batch; the 16 lanes of a lane group are then reduced by
// a fixed xor tree and each A wave writes one partial per clip ([clip][wave][CP],
// summed in order by tail_sum_kernel): bitwise batch- and chunk-invariant.
// SCA, SCB > 0 (f16x2 pair / last-layer instances for fixed dilations, IMM below): the
// roles' tap column steps (A: d, B: sB d; LM: d) at compile time
// LIN (round 6; undilated bf16 two-stream pairs whose LDS pixel is the HBM pixel, PXB ==
// CB: res8's 13-pixel and res26's 20-pixel rows): a stream's A-in rows are one contiguous
// byte range in HBM (clip-major, row-major) and the A-in ring holds them contiguously
// (slot pitch = the row's bytes, NRA a multiple of 1 KiB / gcd), so the DMA is a linear
// copy in 1-KiB pieces into a ring of whole pieces: a row of 1,248 B took two pieces
// (the second 22 % used), a step's ~5 rows 10 pieces; linearly they take 6-7.
template <int NT, int SP, int PPR, int PPW, int NS, bool LM, int FM, int SCA = 0, int SCB = 0, bool LIN = false>
__device__ __forceinline__ void block16p_body(const Block16PArgs& a) {
  using G = G16W<NT, SP, FM>;
  using Q = G16P<NT, SP>;
  constexpr int KSA = G::KSA, CB = G::CB, CP = G::CP, P = Q::P;
  // operand prefetch distance: f16x2 (KSA 14) reads 6 k-steps ahead (7 register sets;
  // measured -3 % on the pair launch against G::PD = 1)
  // TBL (below: f16x2, and the bf16 tap-step instances) reads 6 k-steps ahead too
  // (two streams, NS = 2: two waves per SIMD, 256 registers -- the other wave hides the reads)
  constexpr int PD0 = ((FM == 2 || SCA > 0) && KSA % 7 == 0 && NS == 1) ? 6 : G::PD;
  // NOA operand register sets (a set is re-filled NOA - PD k-steps after the MFMAs that read
  // it: at 1 the ds_read's WAR hazard on the registers the previous k-step's MFMAs read costs
  // s_nops; KSA % NOA == 0 keeps the set of k-step S at S % NOA across m-tiles)
  constexpr int NOA = PD0 + 1;
  constexpr int PD = PD0 > 2 ? PD0 - HONK_PAIR_PDM : PD0;
  constexpr int PXB = Q::PXB;
  constexpr int MAXR = (2 * PPW + PPR - 1) / PPR;  // rows one step's pieces can cover
  static_assert(KSA > PPW + 1, "DMA pieces ride on k-steps 1 .. PPW");
  __shared__ __attribute__((aligned(16))) char lds[g16p_lds_bytes()];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int WPS = LM ? 2 : 4;  // waves per stream
  const int stream = wave / WPS;
  // 0: layer A, 1: layer B.  Two streams (MIX): stream 1's roles are swapped, so each SIMD
  // holds one A wave and one B wave (wave w and w + 4 of a workgroup share a SIMD) instead of
  // two of the same role
  const int role = LM ? 0 : ((wave >> 1) & 1) ^ ((HONK_PAIR_MIX && NS == 2) ? (stream & 1) : 0);
  const int widx = wave & 1;
  const int g = lane >> 4;
  const int i16 = lane & 15;

  // this workgroup's clips, then this stream's share (stream 0 takes the larger half)
  const int GR = gridDim.x;
  const int bid = blockIdx.x;
  // (a device-held clip count -- FM 1, an ordered re-run round -- takes nclips' place: the live
  // clips spread over the grid.  A workgroup then walks fewer clips than the host planned for;
  // plan_pair's lag, ring sizes and pieces per step hold for any shorter stream, and
  // chunk_bytes stays the allocated range.)
  int nclips = a.nclips;
  if constexpr (FM == 1) {
    if (a.live.count) nclips = live_clips(a.live, a.nclips);
  }
  const int w0 = (int)(((long)bid * nclips) / GR);
  const int w1 = (int)(((long)(bid + 1) * nclips) / GR);
  if (w1 <= w0) return;  // whole workgroup, before any barrier
  const int per = (w1 - w0 + NS - 1) / NS;
  const int s0 = min(w0 + stream * per, w1);
  const int s1 = min(s0 + per, w1);
  // the clips the walk covers: the stream's (LM: one clip at a time, set per clip)
  int c0 = s0, c1 = s1;
  const int H = a.H, W = a.W, d = a.d, lgd = a.lgd;
  const int RB = W * CB;
  const unsigned clip_bytes = (unsigned)(H * RB);
  int rows_total = (c1 - c0) * H;
  int total = rows_total * W;
  const int qd = H >> lgd, rem = H & (d - 1);
  const int q1 = qd + 1;
  // TBL (f16x2): the m-tile geometry from a per-wave table of row entries (see
  // refill) instead of a per-lane walk of (class, class row, slots); its invalid taps
  // all point at the zero block's start, so the block spans a whole m-tile's reads
  // (bf16: the tap-step instances, SCA > 0, and the two-stream table instance, SCA = -1)
  constexpr bool TBL = FM == 2 || (FM == 0 && SCA != 0);
  // PADC (TBL, last-layer mode): every ring slot carries zero columns either side of its
  // row (padb bytes), so taps past the map's edge need no check -- measured on res15:
  // the last layer (dilation 16: most taps of a row's edge pixels fall outside) 1.07 ->
  // 1.03 ms; the pairs (dilations <= 8) +1 % (larger slots), so they keep the checks
  constexpr bool PADC = TBL && (LM || SCA > 0);
  const int padb = PADC ? a.padb : 0;
  constexpr int ZB = TBL ? g16p_zb_tbl() : Q::ZB;
  // SHZ: the streams share the zero block, the sink and the zeroed slot (g16p_shared_bytes)
  constexpr bool SHZ = NS > 1 && TBL && !LM;
  // (the zeroed slot spans a slot and, with shared pads, the extra pad its last row reads)
  const int sbase = SHZ ? g16p_shared_bytes(a.slotb + a.ringpad) + stream * g16p_stream_bytes(NS, a.slotb + a.ringpad)
                        : stream * (g16p_lds_bytes() / NS);
  const int ringA = sbase, ringB = sbase + a.NRA * a.slotb;
  const int zoff = SHZ ? 0 : sbase + (a.NRA + a.NRB) * a.slotb + a.ringpad;
  const int dummy = SHZ ? g16p_sink_off(a.slotb + a.ringpad) : zoff + ZB;
  const int nsteps = ((LM ? 1 : per) * H * W + a.lag + P - 1) / P + 1;  // the longer stream's

  // zero block, published before any operand read (the first m-tile's
  // operands load ahead of the step loop)
  if ((wave & (WPS - 1)) == 0) {
    if constexpr (TBL) *(u32x4*)(lds + zoff + lane * 16) = u32x4{0u, 0u, 0u, 0u};
    else *(unsigned*)(lds + zoff + lane * 4) = 0u;
  }
  if constexpr (TBL) {
    // the zeroed slot (see refill) and (PADC) the rings: a slot's pad columns are never written
    // (the DMA fills a row's data bytes and zeros past them, A's epilogue its pixels), so
    // a tap past the map's edge reads a zero there -- no column checks, and a lane group's
    // reads keep the pixel pitch (a zero-block tap among valid ones costs bank conflicts)
    const int zs = SHZ ? 0 : dummy + 1024 + WPS * g16p_tr() * g16p_teb();
    for (int o = ((wave & (WPS - 1)) * 64 + lane) * 16; o < a.slotb + a.ringpad; o += WPS * 1024)
      *(u32x4*)(lds + zs + o) = u32x4{0u, 0u, 0u, 0u};
    const int rings = PADC ? (a.NRA + a.NRB) * a.slotb + a.ringpad : 0;
    for (int o = ((wave & (WPS - 1)) * 64 + lane) * 16; o < rings; o += WPS * 1024)
      *(u32x4*)(lds + sbase + o) = u32x4{0u, 0u, 0u, 0u};
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();

  // the layer's weight operand, resident for the whole launch
  u32x4 wr[G::WP][KSA][NT];
  {
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(role ? a.wB : a.wA), (short)0, G::WP * G::WPART, 0x00020000);
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
          // two waves per SIMD (NS = 2, the bf16 pair): 256 registers per wave.  The walk-based
          // kernel of rounds 3-5 pinned 26-33 fragments and still reloaded spilled values in its
          // step loop (an LLVM partial-spill miscompile at 32 pins, round 4); on the row-table
          // walk (TBL) the wave's state is smaller: 32 fragments pinned (128 AGPRs, the other 10
          // in VGPRs) compile to 120 + 128 registers with no spill at all (round 6).
          // One wave per SIMD: the first 64 fragments (256 AGPRs).
          if ((pt * KSA + s) * NT + n < (NS * WPS > 4 ? 32 : 64)) asm volatile("" : "+a"(wr[pt][s][n]));
        }
  }

  // k-step S, lane group g: chunk c = 4 S + g (MERGE's last step: g - UGA for the lo
  // groups) of the K order (tap, channel chunk); tap(S, g) = c / (2 NT), cc = c mod 2 NT.
  // The lane's operand address of step S is then tb[tap] + 16 cc.  geo() stores
  // tq[t] = tb[t] - 16 (2 NT) t + 16 g per tap, so that every k-step but the last
  // reads tq[tap(S, g)] + 64 S (an immediate): a pure step (one tap) costs nothing,
  // a mixed one (two taps) one select by the lane group -- no per-k-step arithmetic.
  constexpr int CPT = 2 * NT;  // 8-channel chunks per tap
  const int g16 = 16 * g;
  const int hi2 = g >= 2 ? -1 : 0;  // lane groups 2, 3
  // the last k-step (lane groups past the 18 NT chunks, MERGE's mirrored lo groups):
  // all lanes on tap tA(KSA - 1); the lane's address is tq[tA] + lastc
  int lastc;
  {
    constexpr int S = KSA - 1, tA = (4 * S) / CPT;
    int cc[4];
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
      const int gg = (G::MERGE && gi >= G::UGA) ? gi - G::UGA : gi;
      const int c = 4 * S + gg;
      cc[gi] = c < 18 * NT ? c - tA * CPT : 0;
    }
    const int ccg = g == 0 ? cc[0] : g == 1 ? cc[1] : g == 2 ? cc[2] : cc[3];
    lastc = 16 * ccg + 16 * CPT * tA - g16;
  }
  static_assert((4 * (KSA - 1) + 3) / CPT == (4 * (KSA - 1)) / CPT || 4 * (KSA - 1) + 3 >= 18 * NT,
                "the last k-step covers one tap");

  // role constants: the ring the role reads, its taps (sr class rows, sc map columns apart)
  const int ring = role ? ringB : ringA;
  const int nr = role ? a.NRB : a.NRA;
  const int sr = role ? a.sB : 1;
  const int sc = role ? (a.sB << lgd) : d;
  const int scb = sc * PXB;

  // ---- the lane's walk over its m-tiles: stream pixel q, +32 per m-tile ----
  // (w, j, n, c): column, class row, rows of the class, class; rowb: the row's byte
  // offset in the chunk; sR / sO: the row's slot (bytes) in the role's ring / in the
  // A-out ring.  Offsets advance by additions (no integer multiplies in the loop):
  // the next row is dRB further within a class, dcls(n) at a class change (from the
  // class's last row c + (n - 1) d to row c + 1), dclip at a clip change.
  struct Walk {
    int q, w, j, n, c;
    unsigned rowb;
    int sR, sO;
  };
  const unsigned dRB = (unsigned)(RB << lgd);
  const unsigned dclsd = (unsigned)RB - (unsigned)(qd - 1) * dRB, dcls1d = 0u - dRB;  // dcls(q1) - dcls(qd)
  const unsigned dclip = clip_bytes - (unsigned)((d - 1) * RB) - (unsigned)(((d - 1) < rem ? q1 : qd) - 1) * dRB;
  const int ringRb = nr * a.slotb, ringOb = a.NRB * a.slotb, srb = sr * a.slotb;
  auto walk_init = [&](int q0) {
    Walk k;
    k.q = q0;
    const int qs = q0 >= 0 ? q0 : q0 + ((31 - q0) >> 5) * 32;  // first position >= 0
    const int r = qs / W;
    k.w = qs - r * W;
    const int cl = r / H;
    const int rl = r - cl * H;
    if (rl < rem * q1) {
      k.c = rl / q1;
      k.j = rl - k.c * q1;
      k.n = q1;
    } else {
      const int t = rl - rem * q1;
      const int cu = t / qd;
      k.c = rem + cu;
      k.j = t - cu * qd;
      k.n = qd;
    }
    k.rowb = (unsigned)(c0 + cl) * clip_bytes + (unsigned)((k.c + (k.j << lgd)) * RB);
    k.sR = (r % nr) * a.slotb;
    k.sO = (r % a.NRB) * a.slotb;
    return k;
  };
  auto row_adv = [&](Walk& k) {
    const int sR1 = k.sR + a.slotb, sO1 = k.sO + a.slotb;
    k.sR = sR1 == ringRb ? 0 : sR1;
    k.sO = sO1 == ringOb ? 0 : sO1;
    const int j1 = k.j + 1;
    const bool wj = j1 == k.n;                 // next class
    const int c1 = k.c + (wj ? 1 : 0);
    const bool wc = c1 == d;                    // next clip
    // (selects between a computed value and one captured constant only: a ?: on two
    // captured constants becomes a dynamically indexed, scratch-resident closure)
    unsigned inc = dRB;
    const unsigned dcls = dclsd + (k.n == q1 ? dcls1d : 0u);
    inc = wj ? dcls : inc;
    inc = wc ? dclip : inc;
    k.rowb += inc;
    k.j = wj ? 0 : j1;
    k.c = wc ? 0 : c1;
    k.n = k.c < rem ? q1 : qd;
  };
  // rows of >= 32 pixels (W > 32 guaranteed by the row's DMA piece count): an
  // m-tile advance wraps at most one row, done branch-free with the wrap folded
  // into the increments
  constexpr bool WIDE = (PPR - 1) * 1024 >= 32 * PXB;
  auto walk_adv = [&](Walk& k) {
    if constexpr (WIDE) {
      const int w2 = k.w + (k.q >= 0 ? 32 : 0);
      const bool wrap = w2 >= W;
      k.w = wrap ? w2 - W : w2;
      const int sR1 = k.sR + (wrap ? a.slotb : 0), sO1 = k.sO + (wrap ? a.slotb : 0);
      k.sR = sR1 == ringRb ? 0 : sR1;
      k.sO = sO1 == ringOb ? 0 : sO1;
      const int j1 = k.j + (wrap ? 1 : 0);
      const bool wj = j1 == k.n;
      const int c1 = k.c + (wj ? 1 : 0);
      const bool wc = c1 == d;
      unsigned inc = wrap ? dRB : 0u;
      const unsigned dcls = dclsd + (k.n == q1 ? dcls1d : 0u);
      inc = wj ? dcls : inc;
      inc = wc ? dclip : inc;
      k.rowb += inc;
      k.j = wj ? 0 : j1;
      k.c = wc ? 0 : c1;
      k.n = k.c < rem ? q1 : qd;
    } else {
      if (k.q >= 0) {
        k.w += 32;
        while (k.w >= W) {
          k.w -= W;
          row_adv(k);
        }
      }
    }
    k.q += 32;
  };
  // m-tile geometry from the walk: tq[] (see lastc), the pixel's offset in the chunk
  // (0xF0000000: not a pixel) and its LDS offset in the A-out ring.  A tap outside
  // the class-row unit or the map points at the zero block.
  struct MG {
    int tq[9];
    unsigned pix;
    int lo;
  };
  auto geo = [&](const Walk& k) {
    MG m;
    const bool valid = k.q >= 0 && k.q < total;
    int sm = k.sR - srb, sp = k.sR + srb;
    sm = sm < 0 ? sm + ringRb : sm;
    sp = sp >= ringRb ? sp - ringRb : sp;
    const int wb = k.w * PXB + g16;
    const bool rok[3] = {valid && k.j >= sr, valid, valid && k.j + sr < k.n};
    const int rbase[3] = {ring + sm + wb, ring + k.sR + wb, ring + sp + wb};
    const bool cok[3] = {k.w >= sc, true, k.w + sc < W};
    const int zg = zoff + g16;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int t = dy * 3 + dx;
        m.tq[t] = ((rok[dy] && cok[dx]) ? rbase[dy] + (dx - 1) * scb : zg) - 16 * CPT * t;
      }
    m.pix = valid ? k.rowb + (unsigned)(k.w * CB) : 0xF0000000u;
    // (not a stream pixel: A's epilogue writes go to the DMA sink -- no branch)
    m.lo = valid ? ringB + k.sO + k.w * PXB : dummy;
    return m;
  };

  // ---- TBL: the row entries of the wave's next TR stream rows ----
  // Entry of stream row r (slot r mod TR of the wave's table): the LDS bases of the
  // role's ring slots holding tap rows r - sr, r, r + sr (the zeroed slot: outside the
  // row's class or not a row), the row's offset in the chunk (0xF0000000: not a row) and its
  // A-out slot (-1: not a row).  The lane's walk is then (w, r) only, and an m-tile's
  // geometry one 16 + 4-byte table read and ~30 VALU (the walk above: ~75).  The
  // table is private to the wave: refilled (lane l: row tb + l) at the top of a step
  // whose rows would leave it (every ~18 steps on 40-pixel rows).
  constexpr int TR = g16p_tr(), TEB = g16p_teb();
  const int tbl = (SHZ ? sbase + (a.NRA + a.NRB) * a.slotb + a.ringpad : dummy + 1024) + (wave & (WPS - 1)) * (TR * TEB);
  const int zslot = SHZ ? 0 : dummy + 1024 + WPS * (TR * TEB);
  struct WalkT {
    int w, r;
    u32x4 e;  // the row's entry {rb0, rb1, rb2, pix}
    int lo;
    int wb;         // the column's LDS offset in a slot (+ the lane group's chunk)
    bool okl, okr;  // !PADC: the left / right tap columns inside the map
  };
  auto refill = [&](int tb) {
    const int r = tb + lane;
    int rb0 = zslot + padb, rb1 = zslot + padb, rb2 = zslot + padb, lo = -1;
    unsigned pix = 0xF0000000u;
    if (lane < TR && r >= 0 && r < rows_total) {
      const int cl = r / H, rl = r - cl * H;
      int c, j, n;
      if (rl < rem * q1) {
        c = rl / q1;
        j = rl - c * q1;
        n = q1;
      } else {
        const int t = rl - rem * q1, cu = t / qd;
        c = rem + cu;
        j = t - cu * qd;
        n = qd;
      }
      pix = (unsigned)(c0 + cl) * clip_bytes + (unsigned)((c + (j << lgd)) * RB);
      rb1 = ring + (r % nr) * a.slotb + padb;
      if (j >= sr) rb0 = ring + ((r - sr) % nr) * a.slotb + padb;
      if (j + sr < n) rb2 = ring + ((r + sr) % nr) * a.slotb + padb;
      lo = ringB + (r % a.NRB) * a.slotb + padb;
    }
    if (lane < TR) {
      char* e = lds + tbl + (r & (TR - 1)) * TEB;
      *(u32x4*)e = u32x4{(unsigned)rb0, (unsigned)rb1, (unsigned)rb2, pix};
      *(int*)(e + 16) = lo;
    }
  };
  auto floordiv = [](int x, int y) { return x >= 0 ? x / y : -((y - 1 - x) / y); };
  // (role A reads the three row bases only, 12 bytes: it stores nothing to HBM, and a dead
  // fourth element's register was reused at once -- the compiler then drained the LDS queue,
  // the prefetched operand reads ahead of this one included, right behind this read)
  typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
  auto tread = [&](auto rolec, WalkT& k) {
    const char* e = lds + tbl + (k.r & (TR - 1)) * TEB;
    if constexpr (decltype(rolec)::value) {
      k.e = *(const u32x4*)e;
    } else {
      const u32x3 e3 = *(const u32x3*)e;
      k.e = u32x4{e3[0], e3[1], e3[2], 0xF0000000u};
    }
    k.lo = *(const int*)(e + 16);
    k.wb = __mul24(k.w, PXB) + g16;
    if constexpr (!PADC) {
      k.okl = k.w >= sc;
      k.okr = k.w + sc < W;
    }
  };
  auto walk_init_t = [&](auto rolec, int q0) {
    WalkT k;
    k.r = floordiv(q0, W);
    k.w = q0 - k.r * W;
    tread(rolec, k);
    return k;
  };
  // (rows of >= 11 pixels: the instantiated row pitches; WIDE: >= 33)
  constexpr int NWRAP = WIDE ? 1 : 3;
  auto walk_adv_t = [&](auto rolec, WalkT& k) {
    k.w += 32;
#pragma unroll
    for (int i = 0; i < NWRAP; ++i) {
      const bool wrap = k.w >= W;
      k.w = wrap ? k.w - W : k.w;
      k.r += wrap ? 1 : 0;
    }
    tread(rolec, k);
  };
  // per-tap constants: column offset and the tq bias (see lastc)
  int tk[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) tk[t] = (t % 3 - 1) * scb - 16 * CPT * t;
  // tap row DY's three taps (DY = 2: also the pixel's chunk and A-out offsets)
  const int zg0 = zoff + g16;
  // IMM (SCA / SCB > 0, with the pad columns): a tap's column step is a constant, so an
  // m-tile's geometry is three row bases R[dy] (in tq[0..2]) and every operand read is
  // R[dy] + an immediate: no per-tap address arithmetic (9 adds) and no selects of the
  // tq for the mixed k-steps beyond one add (a same-row tap pair) or a bfi + add
  auto scc_of = [](auto rolec) constexpr { return decltype(rolec)::value ? SCB : SCA; };
  auto biasc_of = [](auto rolec) constexpr {
    return (decltype(rolec)::value ? SCB : SCA) * PXB + 96;
  };
  auto geo_row = [&](auto rolec, const WalkT& k, MG& m, auto dyc) {
    constexpr int DY = decltype(dyc)::value;
    constexpr int SCC = scc_of(decltype(rolec){});
    const int rb = (int)k.e[DY] + k.wb;
    if constexpr (PADC && SCC > 0) {
      m.tq[DY] = rb - biasc_of(decltype(rolec){});
    } else if constexpr (PADC) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m.tq[DY * 3 + dx] = rb + tk[DY * 3 + dx];
    } else {
      // an out-of-map column: the zero block at the tap's k-step offsets (1 KiB, see ZB)
      const bool ok[3] = {k.okl, true, k.okr};
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m.tq[DY * 3 + dx] = ok[dx] ? rb + tk[DY * 3 + dx] : zg0;
    }
    if constexpr (DY == 2) {
      m.pix = k.e[3] + (unsigned)__mul24(k.w, CB);
      m.lo = k.lo >= 0 ? k.lo + k.wb - g16 : dummy;
    }
  };
  auto geo_t = [&](auto rolec, const WalkT& k) {
    MG m;
    static_for<3>([&](auto dyc) { geo_row(rolec, k, m, dyc); });
    return m;
  };
  // IMM: the lane constants of the mixed k-steps (lane groups 2, 3 on the next tap: the
  // same tap row, or the next row's first tap) and of the last k-step
  auto lc_same = [&](auto rolec) { return hi2 & (scc_of(decltype(rolec){}) * PXB - 16 * CPT); };
  auto lc_next = [&](auto rolec) { return hi2 & (-2 * scc_of(decltype(rolec){}) * PXB - 16 * CPT); };
  // A-operand offset of k-step S for the lane (64 S rides in the read's immediate)
  auto aoff = [&](auto rolec, const int (&tq)[9], auto stc) {
    constexpr int S = decltype(stc)::value;
    constexpr int tA = (4 * S) / CPT;
    constexpr int SCC = scc_of(decltype(rolec){});
    if constexpr (PADC && SCC > 0) {
      // the base; the immediate is imm_of
      if constexpr (S == KSA - 1) {
        return tq[tA / 3] + lastc - 16 * CPT * tA;
      } else {
        constexpr int tB = (4 * S + 3) / CPT;
        if constexpr (tA == tB) {
          return tq[tA / 3];
        } else if constexpr (tA / 3 == tB / 3) {
          return tq[tA / 3] + lc_same(rolec);
        } else {
          return ((tq[tB / 3] & hi2) | (tq[tA / 3] & ~hi2)) + lc_next(rolec);
        }
      }
    } else if constexpr (S == KSA - 1) {
      return tq[tA] + lastc - 64 * S;
    } else {
      constexpr int tB = (4 * S + 3) / CPT;
      if constexpr (tA == tB) {
        return tq[tA];
      } else {
        // lane groups >= GS on tap tB: a bitwise select (one v_bfi_b32; a ?: on the two
        // elements becomes a select of their addresses and a scratch-resident tq)
        constexpr int GS = CPT * tB - 4 * S;
        static_assert(GS == 2, "NT = 3: every mixed k-step splits its lane groups 2 + 2");
        return (tq[tB] & hi2) | (tq[tA] & ~hi2);
      }
    }
  };

  // IMM: the read's immediate for k-step S (tap tA's column step and k-step offset, + the
  // bias taken off the row bases; >= 64: every tap's first k-step S has 64 S >= 96 t - 32)
  auto imm_of = [](auto rolec, auto stc) constexpr {
    constexpr int S = decltype(stc)::value;
    constexpr int tA = (4 * S) / CPT;
    constexpr int SCC = decltype(rolec)::value ? SCB : SCA;
    constexpr int B = SCC * PXB + 96;
    if constexpr (S == KSA - 1) return B + (tA % 3 - 1) * SCC * PXB;
    else return B + (tA % 3 - 1) * SCC * PXB - 16 * CPT * tA + 64 * S;
  };

  u32x4 oa[NOA][SP];
  auto load_a = [&](auto rolec, const int (&tq)[9], auto stc, u32x4 (&o)[SP]) {
    constexpr int S = decltype(stc)::value;
    const int off = aoff(rolec, tq, stc);
    if constexpr (PADC && scc_of(decltype(rolec){}) > 0) {
      constexpr int IMM = imm_of(decltype(rolec){}, stc);
      static_assert(IMM >= 0 && IMM < 65536, "IMM: ds_read offset range");
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) o[pt] = *(const u32x4*)(lds + off + IMM + pt * CP * 2);
    } else {
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) o[pt] = *(const u32x4*)(lds + off + 64 * S + pt * CP * 2);
    }
  };

  // ---------------- deferred epilogue state (both roles) ----------------
  // A step runs two m-tiles: m-tile `it` (0, 1) keeps its accumulators, residual
  // runs (B) and geometry in set `it`, so the pending m-tile's state is simply the
  // other set -- nothing is copied between m-tiles
  f32x4 accs[2][NT];
  uint4 rvs[2][G::NRF][SP];     // B: residual runs of the m-tile of each parity
  unsigned ppix = 0xF0000000u;  // B: pending pixel's offset in the chunk
  int plo = dummy;              // A: pending pixel's A-out LDS offset (the sink if not a stream pixel,
                                //    and before the first m-tile: its "pending" epilogue is empty)
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int n = 0; n < NT; ++n) accs[q][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int f = 0; f < G::NRF; ++f)
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) rvs[q][f][pt] = uint4{0u, 0u, 0u, 0u};
  }
  const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.R, (short)0, a.chunk_bytes, 0x00020000);

  constexpr int NSTO = LM ? 0 : G::NS;  // stores (B) / LDS writes (A) per m-tile
  constexpr int ELAST = LM ? NT - 1 : G::store_step(NSTO - 1);
  f32x4 csum[NT];  // LM: the lane's channel sums over its pixels of the clip
#pragma unroll
  for (int n = 0; n < NT; ++n) csum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int KE = (KSA - ELAST - 2 >= 2) ? KSA - ELAST - 2 : 2;
  constexpr int KW = 4;                  // k-step of the walk's advance
  constexpr int KG = KSA - 1 - PD - 1;   // k-step of the next m-tile's geometry
  static_assert(KG > KW && KG + PD < KSA, "walk schedule");
  // TBL: the walk (and its table read) on k-step 1, the epilogue's half steps from
  // k-step 2, then the three tap rows of the next m-tile's geometry on one k-step each
  // (measured slower than KW / KG / KE on the f16x2 pair: 2.17 vs 2.08 ms; kept off)
  constexpr bool BAL = false;
  constexpr int NHS = 2 * ELAST + 2;
  constexpr int KWT = PD > 2 ? 0 : 1, KET = PD > 2 ? 5 : 2, KGT = PD > 2 ? 2 : KET + NHS;
  static_assert(!(TBL && BAL) || (KGT + 2 + PD < KSA && KET + NHS <= KSA && KWT < KGT), "table walk schedule");

  typename ActT<FM>::V4 h[SP][NT];
  // output i of the pending m-tile (its tiles finished): B stores it over the
  // residual, A writes it into the A-out ring
  auto epi_store = [&](auto rolec, auto ic) {
    constexpr bool ISB = decltype(rolec)::value;
    constexpr int I = decltype(ic)::value;
    if constexpr (I < G::NPS) {
      constexpr int pr = I / SP, pt = I % SP;
      const u32x2 lo = __builtin_bit_cast(u32x2, h[pt][2 * pr]), hi = __builtin_bit_cast(u32x2, h[pt][2 * pr + 1]);
      const u32x4 v4{lo[0], lo[1], hi[0], hi[1]};
      if constexpr (ISB) {
        __builtin_amdgcn_raw_buffer_store_b128(v4, rrs, ppix + 16 * g, 64 * pr + pt * CP * 2, 0);
      } else {
        *(u32x4*)(lds + plo + 16 * g + 64 * pr + pt * CP * 2) = v4;
      }
    } else {
      constexpr int pt = I - G::NPS;
      const u32x2 v2 = __builtin_bit_cast(u32x2, h[pt][NT - 1]);
      if constexpr (ISB) {
        __builtin_amdgcn_raw_buffer_store_b64(v2, rrs, ppix + 8 * g, 64 * (NT / 2) + pt * CP * 2, 0);
      } else {
        *(u32x2*)(lds + plo + 8 * g + 64 * (NT / 2) + pt * CP * 2) = v2;
      }
    }
  };
  // epilogue step E of the pending m-tile: E < NT finishes out-tile E (ReLU,
  // [B: + residual], bf16 hi/lo split); output i goes out at store_step(i)
  auto epi_step = [&](auto rolec, auto ec, auto pendc) {
    constexpr bool ISB = decltype(rolec)::value;
    constexpr int E = decltype(ec)::value;
    constexpr int PQ = decltype(pendc)::value;  // the pending m-tile's set
    f32x4 (&accp)[NT] = accs[PQ];
    uint4 (&rv)[G::NRF][SP] = rvs[PQ];
    if constexpr (E < NT && !ISB && !LM && FM == 2 && HONK_PAIR_PKRELU) {
      // A (f16x2): round to fp16 first, then ReLU on the packed pair -- relu and RNE commute
      // (maximum(x, +0) keeps a NaN, maps -0 and every x <= 0 to +0 either way), so this is
      // bit-for-bit relu-then-convert in 2 v_cvt_pk_f16_f32 + 2 v_pk_maximum3_f16 per
      // out-tile instead of 4 v_maximum3_f32 + 2 converts
      constexpr int n = E;
      const f16x4 hv{(_Float16)accp[n][0], (_Float16)accp[n][1], (_Float16)accp[n][2], (_Float16)accp[n][3]};
      h[0][n] = __builtin_bit_cast(typename ActT<FM>::V4, __builtin_elementwise_maximum(hv, f16x4{0, 0, 0, 0}));
    } else if constexpr (E < NT) {
      constexpr int n = E;
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = relu_acc(accp[n][k]);
      if constexpr (ISB) {
        constexpr int f = n >> 1, e0 = (n < (NT & ~1)) ? (n & 1) * 4 : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = e0 + k;
          // (the parts summed from the first: a 0.f start costs an add of +0 per value)
          if constexpr (SP == 1) {
            v[k] = add_res<FM>(v[k], rv[f][0][e >> 1], e);
          } else {
            const float r = act_dec<FM>(rv[f][0][e >> 1], e) + act_dec<FM>(rv[f][1][e >> 1], e);
            v[k] += r;
          }
        }
      }
      if constexpr (LM) {
        const bool ok = plo != dummy;  // a stream pixel
#pragma unroll
        for (int k = 0; k < 4; ++k) csum[n][k] += ok ? v[k] : 0.f;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          h[0][n][k] = (typename ActT<FM>::T)v[k];
          if constexpr (SP == 2) h[SP - 1][n][k] = (__bf16)(v[k] - (float)h[0][n][k]);
        }
      }
    }
    static_for<NSTO>([&](auto ic) {
      if constexpr (G::store_step(decltype(ic)::value) == E) epi_store(rolec, ic);
    });
  };
  // TBL: the same epilogue in half steps (HS = 2 n + half: values 2 half, 2 half + 1
  // of out-tile n; output i at half step 2 store_step(i) + 1), so that no k-step
  // carries more VALU work than its MFMAs hide (two per MFMA)
  auto epi_half = [&](auto rolec, auto hc, auto pendc) {
    constexpr bool ISB = decltype(rolec)::value;
    constexpr int HS = decltype(hc)::value;
    constexpr int PQ = decltype(pendc)::value;
    if constexpr (HS < 2 * NT) {
      constexpr int n = HS / 2, k0 = 2 * (HS % 2);
      f32x4 (&accp)[NT] = accs[PQ];
      uint4 (&rv)[G::NRF][SP] = rvs[PQ];
#pragma unroll
      for (int k = k0; k < k0 + 2; ++k) {
        float v = relu_acc(accp[n][k]);
        if constexpr (ISB) {
          constexpr int f = n >> 1, e0 = (n < (NT & ~1)) ? (n & 1) * 4 : 0;
          const int e = e0 + k;
          if constexpr (SP == 1) {
            v = add_res<FM>(v, rv[f][0][e >> 1], e);
          } else {
            const float r = act_dec<FM>(rv[f][0][e >> 1], e) + act_dec<FM>(rv[f][1][e >> 1], e);
            v += r;
          }
        }
        if constexpr (LM) {
          csum[n][k] += plo != dummy ? v : 0.f;
        } else {
          h[0][n][k] = (typename ActT<FM>::T)v;
          if constexpr (SP == 2) h[SP - 1][n][k] = (__bf16)(v - (float)h[0][n][k]);
        }
      }
    }
    static_for<NSTO>([&](auto ic) {
      if constexpr (2 * G::store_step(decltype(ic)::value) + 1 == HS) epi_store(rolec, ic);
    });
  };

  auto res_loads = [&](uint4 (&rvn)[G::NRF][SP], unsigned po) {
#pragma unroll
    for (int f = 0; f < G::NRF; ++f)
#pragma unroll
      for (int pt = 0; pt < SP; ++pt) {
        if (f < NT / 2) {
          rvn[f][pt] =
              __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rrs, po + 16 * g, 64 * f + pt * CP * 2, 0));
        } else {
          const u32x2 t =
              __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rrs, po + 8 * g, 64 * f + pt * CP * 2, 0));
          rvn[f][pt] = uint4{t[0], t[1], 0u, 0u};
        }
      }
  };

  // ---------------- A-in staging (A waves; scalar) ----------------
  // Stream rows enter the A-in ring in order; F(k) = the last row needed by A's
  // band k + 1 and by the first m-tiles of band k + 2 (whose first k-steps load
  // before the barrier): pixel (k + 2) P + 31's row + 1.  Rows (F(k-1), F(k)]
  // are loaded at step k; piece p = widx + 2 i of a step covers 1 KiB part p % PPR
  // of row F(k-1) + 1 + p / PPR.  A row cursor tracks (clip, class, class row).
  // The slot holds the row at the padded pitch PXB: lane l of part t fills slot
  // chunk 64 t + l, i.e. pixel (64 t + l) / (PXB / 16), 16-B chunk (64 t + l) %
  // (PXB / 16) of the HBM row, or zeros (a pad chunk, or past the row).
  // The cursor carries the row's byte offset in the chunk, (c0 + clip) clip_bytes + (c + j d) RB,
  // and its slot's byte offset in the ring, both advanced by additions as the lane walk's
  // rowb / sR are (dRB within a class, dcls(n) at a class change, dclip at a clip change): no
  // integer multiplies per step.
  struct RowCur {
    int c, j, n;
    unsigned off;
    int slot;
  };
  const int ringAb = a.NRA * a.slotb;
  // advance by one row where `by` is 1, not at all where it is 0 -- straight-line, the wrap
  // conditions folded into the increments as in walk_adv (j < n, c < d and slot < ringAb hold
  // on entry, so no wrap fires without the advance)
  auto cur_adv = [&](RowCur& r, int by) {
    const int s1 = r.slot + (by ? a.slotb : 0);
    r.slot = s1 == ringAb ? 0 : s1;
    const int j1 = r.j + by;
    const bool wj = j1 == r.n;   // next class
    const int c1 = r.c + (wj ? 1 : 0);
    const bool wc = c1 == d;     // next clip
    unsigned inc = by ? dRB : 0u;
    const unsigned dcls = dclsd + (r.n == q1 ? dcls1d : 0u);
    inc = wj ? dcls : inc;
    inc = wc ? dclip : inc;
    r.off += inc;
    r.j = wj ? 0 : j1;
    r.c = wc ? 0 : c1;
    r.n = r.c < rem ? q1 : qd;
  };
  // per part: the lane's byte offset in the HBM row (16-bit, 0xffff: zeros)
  unsigned psrc[(PPR + 1) / 2];
#pragma unroll
  for (int i = 0; i < (PPR + 1) / 2; ++i) psrc[i] = 0;
#pragma unroll
  for (int t = 0; t < PPR; ++t) {
    const int ch = 64 * t + lane, px = ch / (PXB / 16), wi = ch - px * (PXB / 16);
    const unsigned v = (px < W && wi < CB / 16) ? (unsigned)(px * CB + wi * 16) : 0xffffu;
    psrc[t >> 1] |= v << (16 * (t & 1));
  }
  auto dma = [&](unsigned off, int slot, auto pac, auto pbc, bool ok) {
    constexpr int PA = decltype(pac)::value, PB = decltype(pbc)::value;
    const int part = widx ? PB : PA;
    const unsigned va = (psrc[PA >> 1] >> (16 * (PA & 1))) & 0xffffu, vb = (psrc[PB >> 1] >> (16 * (PB & 1))) & 0xffffu;
    const unsigned v = widx ? vb : va;
    const int dst = ok ? ringA + slot + padb + part * 1024 : dummy;
    // not ok: an offset past the chunk (< 0xF0000000 bytes) loads zeros into the sink
    // (one resource: a ?: on two resources becomes a scratch-resident select)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rrs,
                                             (__attribute__((address_space(3))) void*)(lds + __builtin_amdgcn_readfirstlane(dst)),
                                             16, (v == 0xffffu || !ok) ? 0xF0000000u : off + v, 0, 0, 0);
  };
  // frontier pixel (k + 2) P + 31 as (row, column), advanced by P per step
  const int PW = P / W, PR = P - PW * W;
  int frow = (P + 31) / W, fcol = (P + 31) - ((P + 31) / W) * W;  // k = -1
  auto frontier = [&]() { return frow + 1 < rows_total - 1 ? frow + 1 : rows_total - 1; };
  RowCur rc{0, 0, rem > 0 ? q1 : qd, (unsigned)c0 * clip_bytes, 0};  // the next row to load (row 0)
  // LM: the walk restarts at each clip (run_role's prologue then derives the clip's first
  // descriptors from the reset cursor)
  auto restart = [&]() {
    rows_total = (c1 - c0) * H;
    total = rows_total * W;
    frow = (P + 31) / W;
    fcol = (P + 31) - ((P + 31) / W) * W;
    rc = RowCur{0, 0, rem > 0 ? q1 : qd, (unsigned)c0 * clip_bytes, 0};
    plo = dummy;
    ppix = 0xF0000000u;
  };
  // The step's DMA descriptors: nnew rows (F(k-1), F(k)], row m at chunk offset roff[m] into
  // ring offset rslot[m] (entries m >= nnew are not used: their pieces go to the sink).  They
  // are software-pipelined: step k + 1's are derived during step k (step 0's in run_role's
  // prologue), straight-line and without multiplies, so no step waits for its own.
  int fprev = 0, nnew = 0;
  unsigned roff[MAXR];
  int rslot[MAXR];
  static_assert(MAXR + 2 < KSA, "desc_row(m) rides on k-step 2 + m");
  // (The arithmetic depends on nothing but loop-carried scalars, so where it lands in the
  // step's block is instruction selection's choice, whatever k-step calls it: the head of the
  // block, ahead of k-step 0's first sched_barrier.  Being a step ahead it is needed nowhere
  // in this step, so DTOP opens k-steps 0 and 1 to it and the scheduler spreads it under their
  // MFMAs.  Pinning it to the second m-tile's k-steps with empty asm statements on the state
  // was tried: the statements pushed the first m-tile's MFMAs behind them -- not kept.)
  auto desc_front = [&]() {  // the frontier of the next step and its count of new rows
    fcol += PR;
    frow += PW;
    const bool wrap = fcol >= W;
    fcol -= wrap ? W : 0;
    frow += wrap ? 1 : 0;
    const int fcur = frontier();
    nnew = fcur - fprev;
    fprev = fcur;
  };
  auto desc_row = [&](int m) {  // row m of the next step; the cursor ends nnew (<= MAXR) rows on
    roff[m] = rc.off;
    rslot[m] = rc.slot;
    cur_adv(rc, m < nnew ? 1 : 0);
  };
  // LIN: pieces issued so far, this step's new pieces start at ring piece lpb and HBM byte
  // lsrc (the stream's byte lsb0 + 1 KiB x pieces issued)
  static_assert(!LIN || (!LM && TBL && !PADC), "LIN: the two-stream row-table pair");
  const unsigned lsb0 = (unsigned)c0 * clip_bytes;
  const int lnpr = LIN ? a.NRA * a.slotb / 1024 : 1;  // ring pieces
  const int lptot = LIN ? (rows_total * RB + 1023) / 1024 : 0;
  int lpdone = 0, lpb = 0;
  unsigned lsrc = 0;
  auto lin_need = [&](int f) {  // pieces covering rows 0 .. f of the stream
    const int p = ((f + 1) * RB + 1023) / 1024;
    return p < lptot ? p : lptot;
  };
  // LIN's descriptors of the next step (pipelined as desc_front / desc_row are): nnew pieces
  // from ring piece lpb (advanced by the previous step's count, one wrap: a step's pieces are
  // fewer than the ring's -- lin_dma wraps lpb + j the same way) and HBM byte lsrc
  auto lin_next = [&]() {
    fcol += PR;
    frow += PW;
    const bool wrap = fcol >= W;
    fcol -= wrap ? W : 0;
    frow += wrap ? 1 : 0;
    const int need = lin_need(frontier());
    lpb += nnew;
    lpb -= lpb >= lnpr ? lnpr : 0;
    lsrc += (unsigned)nnew * 1024u;
    nnew = need - lpdone;
    lpdone = need;
  };
  auto lin_dma = [&](int j, int nnew) {
    const bool ok = j < nnew;
    int rp = lpb + j;
    rp = rp >= lnpr ? rp - lnpr : rp;
    const int dst = ok ? ringA + rp * 1024 : dummy;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rrs, (__attribute__((address_space(3))) void*)(lds + __builtin_amdgcn_readfirstlane(dst)), 16,
        ok ? lsrc + (unsigned)j * 1024u + (unsigned)lane * 16u : 0xF0000000u, 0, 0, 0);
  };
  // (The A waves stream the A-in rows.  Moving the step's pieces to the B waves measured
  // slower -- the four pieces cost B ~420 cycles where they cost A ~300, pair launch 2.03 vs
  // 2.01 ms -- and that variant is gone.)

  // the k-step of the first m-tile that issues DMA piece i, as a map S -> i (-1: none):
  // pieces DSP k-steps apart from k-step 1 (DSP = 1: back to back; 2, 3, 4 measured the
  // same or up to 2 % slower on the f16x2 pair: spacing does not lower a piece's cost)
  constexpr int DSP = 1;
  auto dma_piece = [](int S) constexpr {
    return (S >= 1 && (S - 1) % DSP == 0 && (S - 1) / DSP < PPW) ? (S - 1) / DSP : -1;
  };
  static_assert(1 + DSP * (PPW - 1) < KSA, "DMA pieces inside the first m-tile");
  // B's vector-memory operations issued after the pending m-tile's residual loads (its
  // k-step 0) and before the pending epilogue's first use of them (this m-tile's k-step KE):
  // the NSTO stores that went out during the pending m-tile (k-steps >= KE) and this m-tile's
  // residual loads -- every store of this m-tile follows that first use (store_step >= 1).
  // One wait for all but these ahead of the first use, and the compiler's waitcnt pass finds
  // every later use of a residual register satisfied: it placed a wait per use (counts it
  // cannot bound across the loop's back edge, most of them no-ops that still take an issue slot).
  constexpr int VM_AFTER_RES = NSTO + G::NRL;
  static_assert(G::store_step(0) >= 1 || NSTO == 0, "no store ahead of the first residual use");
  // One m-tile: KSA k-steps of PRODUCTS x NT MFMAs on the tap bases of `cur`; the
  // operands of step S + PD (or of the next m-tile) load under step S's MFMAs.
  // k-step KW advances the walk, KG derives the next m-tile's geometry; the
  // pending epilogue runs from k-step KE; A's first m-tile of a step issues the
  // step's DMA pieces on k-steps 1 .. 8; B loads this m-tile's residual at k-step 0.
  auto run_mtile = [&](auto rolec, auto parc, const MG& cur, MG& nxt, auto& wk, int nnew) {
    constexpr bool ISB = decltype(rolec)::value;
    constexpr int PAR = decltype(parc)::value;  // this m-tile's set; the pending one is 1 - PAR
    constexpr bool FIRST = PAR == 0;
    f32x4 (&acc)[NT] = accs[PAR];
    static_for<KSA>([&](auto stc) {
      constexpr int S = decltype(stc)::value;
      constexpr int SN = S + PD;
      if constexpr (SN < KSA) load_a(rolec, cur.tq, KStep<SN>{}, oa[SN % NOA]);
      else load_a(rolec, nxt.tq, KStep<SN - KSA>{}, oa[SN % NOA]);
      // the operand reads go out ahead of this step's MFMAs (left to itself the
      // scheduler sinks them below most of the step and then waits on them)
      // (DTOP: A's k-steps 0 and 1 of a step form one scheduling region with the head of the
      // step's block, where the next step's DMA descriptors land -- see desc_front)
      constexpr bool DTOP = HONK_PAIR_DTOP && !ISB && FIRST;
      if constexpr (!(DTOP && S <= 1)) __builtin_amdgcn_sched_barrier(0);
      // the step's other work (walk, geometry, residual loads, DMA, epilogue) issues
      // between its MFMAs (pattern at the end of the step): one wave per SIMD, so VALU
      // work bunched ahead of the MFMAs would leave the matrix pipe idle
      if constexpr (ISB && S == 0) res_loads(rvs[PAR], cur.pix);
      if constexpr (TBL && BAL) {
        if constexpr (S == KWT) walk_adv_t(rolec, wk);
        if constexpr (S >= KGT && S < KGT + 3) geo_row(rolec, wk, nxt, std::integral_constant<int, S - KGT>{});
      } else if constexpr (TBL) {
        if constexpr (S == KW) walk_adv_t(rolec, wk);
        if constexpr (S == KG) nxt = geo_t(rolec, wk);
      } else {
        if constexpr (S == KW) walk_adv(wk);
        if constexpr (S == KG) nxt = geo(wk);
      }
      const u32x4 (&ac)[SP] = oa[S % NOA];
      constexpr int NPROD = S == KSA - 1 ? G::NPROD_LAST : G::PRODUCTS;
      static_for<NPROD>([&](auto tc) {
        constexpr int T = decltype(tc)::value;
        constexpr int WP = G::wpart(T), XP = G::xpart(T);
        static_for<NT>([&](auto nc) {
          constexpr int N = decltype(nc)::value;
          mfma_w<S == 0 && T == 0, FM == 2>(acc[N], wr[WP][S][N], ac[XP]);
        });
      });
      if constexpr (LIN && !ISB && FIRST && dma_piece(S) >= 0) {
        lin_dma(2 * dma_piece(S) + widx, nnew);
      } else if constexpr (!ISB && FIRST && dma_piece(S) >= 0) {
        constexpr int i = dma_piece(S);  // this wave's piece p = widx + 2 i: row (p / PPR), part p % PPR
        constexpr int ra = (2 * i) / PPR, rb = (2 * i + 1) / PPR;
        constexpr int pa = (2 * i) % PPR, pb = (2 * i + 1) % PPR;
        const int rr = widx ? rb : ra;
        dma(widx ? roff[rb] : roff[ra], widx ? rslot[rb] : rslot[ra], std::integral_constant<int, pa>{},
            std::integral_constant<int, pb>{}, rr < nnew);
      }
      // the next step's DMA descriptors (scalar; see desc_front for where they land)
      if constexpr (!ISB && !FIRST) {
        if constexpr (LIN) {
          if constexpr (S == 1) lin_next();
        } else {
          if constexpr (S == 1) desc_front();
          if constexpr (S >= 2 && S < 2 + MAXR) desc_row(S - 2);
        }
      }
      if constexpr (TBL && BAL) {
        if constexpr (S >= KET && S < KET + NHS)
          epi_half(rolec, std::integral_constant<int, S - KET>{}, std::integral_constant<int, 1 - PAR>{});
      } else {
        static_for<ELAST + 1>([&](auto ec) {
          constexpr int E = decltype(ec)::value;
          if constexpr ((KE + E < KSA ? KE + E : KSA - 1) == S) {
            if constexpr (ISB && E == 0) wait_vmcnt<VM_AFTER_RES>();
            epi_step(rolec, ec, std::integral_constant<int, 1 - PAR>{});
          }
        });
      }
      if constexpr (DTOP && S <= 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // the operand read first
      static_for<NPROD * NT>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // then up to two VALU
        __builtin_amdgcn_sched_group_barrier(0x004, (DTOP && S <= 1) ? 5 : 2, 0);  // and up to two SALU
      });
      if constexpr (!(DTOP && S == 0)) __builtin_amdgcn_sched_barrier(0);
    });
  };

  auto run_role = [&](auto rolec) {
    constexpr bool ISB = decltype(rolec)::value;
    if constexpr (!ISB) {
      fprev = frontier();
      nnew = 0;
    }
    if constexpr (LIN && !ISB) {
      // prologue: the pieces of rows 0 .. F(-1), the two A waves alternating
      lpdone = lin_need(fprev);
      for (int p = widx; p < lpdone; p += 2)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rrs, (__attribute__((address_space(3))) void*)(lds + __builtin_amdgcn_readfirstlane(ringA + p * 1024)), 16,
            lsb0 + (unsigned)p * 1024u + (unsigned)lane * 16u, 0, 0, 0);
      // step 0's descriptors
      lpb = lpdone % lnpr;
      lsrc = lsb0 + (unsigned)lpdone * 1024u;
      lin_next();
    } else if constexpr (!ISB) {
      // prologue: rows 0 .. F(-1) (A's band 0, its halo row and band 1's first m-tiles)
      for (int row = 0; row <= fprev; ++row) {
        if ((row & 1) == widx) {
          const unsigned ro = rc.off;
          const int so = ringA + rc.slot + padb;
#pragma unroll
          for (int t = 0; t < PPR; ++t) {
            const unsigned v = (psrc[t >> 1] >> (16 * (t & 1))) & 0xffffu;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rrs, (__attribute__((address_space(3))) void*)(lds + __builtin_amdgcn_readfirstlane(so + t * 1024)), 16,
                v == 0xffffu ? 0xF0000000u : ro + v, 0, 0, 0);
          }
        }
        cur_adv(rc, 1);
      }
      // step 0's descriptors
      desc_front();
#pragma unroll
      for (int m = 0; m < MAXR; ++m) desc_row(m);
    }
    const int q0w = (ISB ? -a.lag - P : 0) + 16 * widx;  // the wave's first m-tile
    int qlim = 0;  // TBL: the first stream pixel past the wave's table
    if constexpr (TBL) {
      const int tb = floordiv(q0w, W);
      refill(tb);
      qlim = (tb + TR) * W;
    }
    auto wk = [&]() {
      if constexpr (TBL) return walk_init_t(rolec, q0w + i16);
      else return walk_init(q0w + i16);
    }();
    MG mgs[2];
    if constexpr (TBL) mgs[0] = geo_t(rolec, wk);
    else mgs[0] = geo(wk);
    // B: the weight loads have landed.  (B's loop never waits for all of its vector-memory
    // operations, so the compiler cannot tell and kept a vmcnt wait in front of the first use
    // of every VGPR-resident weight fragment, in every step.  A waits at its first barrier.)
    if constexpr (ISB) wait_vmcnt<0>();
    for (int k = 0; k < nsteps; ++k) {
      // step barrier: this wave's DMA pieces landed (A), A-out writes visible
      // (the asm memory clobbers keep the compiler from moving LDS accesses across the
      // barrier: __builtin_amdgcn_s_barrier alone is not a memory fence to it)
      asm volatile("" ::: "memory");
      if constexpr (!ISB) wait_vmcnt<0>();
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if constexpr (TBL) {
        // the step's m-tiles and the next step's first (geometry at this step's KG)
        const int qs = q0w + k * P;
        if (qs + P + 15 >= qlim) {
          const int tb = floordiv(qs, W);
          refill(tb);
          qlim = (tb + TR) * W;
        }
      }
      // the first m-tile's first operands (later m-tiles' load under the previous one)
      if (k == 0) static_for<PD>([&](auto stc) { load_a(rolec, mgs[0].tq, stc, oa[decltype(stc)::value]); });
      // (A: this step's DMA descriptors -- nnew, roff / rslot or LIN's lpb / lsrc -- stand
      // ready: the previous step's second m-tile, or the prologue, derived them)
      static_for<2>([&](auto itc) {
        constexpr int IT = decltype(itc)::value;
        run_mtile(rolec, std::integral_constant<int, IT>{}, mgs[IT], mgs[1 - IT], wk, nnew);
        // this m-tile becomes the pending epilogue
        ppix = mgs[IT].pix;
        plo = mgs[IT].lo;
      });
    }
    wait_vmcnt<0>();
    static_for<ELAST + 1>([&](auto ec) { epi_step(rolec, ec, std::integral_constant<int, 1>{}); });
  };

  if constexpr (LM) {
    for (int ci = 0; ci < per; ++ci) {
      c0 = s0 + ci;
      c1 = c0 < s1 ? c0 + 1 : c0;  // past the stream's clips: a pass over no pixels (common barriers)
      restart();
      // the previous clip's last operand reads are done before this clip's rows enter the ring
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      run_role(std::integral_constant<bool, false>{});
      // the clip's partial: lane group g's 16 pixels by a fixed xor tree, then one
      // 16-B store per out-tile from lane i16 = 0
      float* cs = a.chsum + ((size_t)(c0 < c1 ? c0 : 0) * 2 + widx) * CP;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        f32x4 c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c[k] = sum16_dpp(csum[n][k]);
        }
        if (c0 < c1 && i16 == 0) *(f32x4*)(cs + co16(NT, n, 4 * g)) = c;
        csum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  } else {
    if (role == 0) run_role(std::integral_constant<bool, false>{});
    else run_role(std::integral_constant<bool, true>{});
  }
}

template <int NT, int SP, int PPR, int PPW, int NS, int FM = (SP == 2 ? 1 : 0), int SCA = 0, int SCB = 0,
          bool LIN = false>
__global__ __launch_bounds__(256 * NS, 1) void block16p_kernel(Block16PArgs a) {
  block16p_body<NT, SP, PPR, PPW, NS, false, FM, SCA, SCB, LIN>(a);
}

// the last (odd) layer with fused channel sums: LM of block16p_body
template <int NT, int SP, int PPR, int PPW, int NS, int FM = (SP == 2 ? 1 : 0), int SCL = 0>
__global__ __launch_bounds__(128 * NS, 1) void block16l_kernel(Block16PArgs a) {
  block16p_body<NT, SP, PPR, PPW, NS, true, FM, SCL, SCL>(a);
}
