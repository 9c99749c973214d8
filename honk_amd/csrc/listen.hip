// The last stage of /listen on gfx950 (honk_listen_decide_f32): per window the label and the
// probability that softmax -> argmax / max give, per segment of windows (a recording of a batch,
// a stream of a tick) the answer ListenEndpoint.POST builds from them -- the summed probability
// and the count per label, and the first window that carries the keyword.
//
// Two launches on the stream, rows then segments; no workspace, no float atomics, and within a
// launch no location is written by one workgroup and read by another.
#include "common.h"

#include <cmath>

namespace honk {
namespace listen {

constexpr int ROW_THREADS = 256;  // 4 waves, each holding 64 / G rows
constexpr int SEG_THREADS = 256;  // one workgroup per segment

// One label per lane, a row per group of G lanes (G the power of two >= n_labels, so a wave
// holds 64 / G whole rows); lanes j >= n_labels of a group and the groups past row n hold -inf.
//   max / first argmax: an xor butterfly over the group on (value, index), ties to the lower
//     index -- both are exact, so the order of the butterfly does not matter;
//   the sum: every lane of the group adds the group's exp terms in ascending j (n_labels
//     cross-lane reads), so the rounding is that of the sequential loop whatever the packing;
//   a row whose IEEE softmax is NaN (a NaN, a +inf, or nothing above -inf): label 0, prob NaN.
// A row's lanes read and write that row only: its result does not depend on n or its neighbours.
template <int G>
__global__ __launch_bounds__(ROW_THREADS) void rows_kernel(const float* __restrict__ logits, int64_t n, int n_labels,
                                                           int32_t* __restrict__ label, float* __restrict__ prob) {
  const int lane = threadIdx.x & 63;
  const int j = lane & (G - 1);
  const int base = lane - j;
  const int64_t r = ((int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6)) * (64 / G) + lane / G;
  const bool live = r < n && j < n_labels;
  const float z = live ? logits[r * n_labels + j] : -INFINITY;
  // (fmaxf would swallow a NaN: the rows that hold one are told apart first)
  const unsigned long long groups = __ballot(z != z || z == INFINITY);
  const unsigned long long mine = (G == 64 ? ~0ull : ((1ull << G) - 1)) << base;
  float m = z;
  int arg = j;
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) {
    const float om = __shfl_xor(m, o);
    const int oa = __shfl_xor(arg, o);
    const bool take = om > m || (om == m && oa < arg);
    m = take ? om : m;
    arg = take ? oa : arg;
  }
  const bool nan_row = (groups & mine) != 0 || m == -INFINITY;
  // z - m: finite or -inf wherever the row is not a NaN row (m is finite there), and expf(-inf) = 0
  const float e = expf(z - m);
  float s = 0.f;
  for (int k = 0; k < n_labels; ++k) s += __shfl(e, base + k);
  if (j == 0 && r < n) {
    label[r] = nan_row ? 0 : arg;
    prob[r] = nan_row ? NAN : 1.f / s;
  }
}

// Segment s = windows [window0[s], window0[s + 1]) (each entry clamped to [0, n]; a table that
// decreases gives an empty segment): one workgroup, its threads striding the windows.
// A finite prob is a multiple of 2^-29 within [2^-6, 1] (1 / a sum of at most 64 terms <= 1), so
// prob * 2^29 is an integer below 2^30 and a segment's sum of at most 2^23 of them stays below
// 2^53: the sums are taken as 64-bit INTEGERS by LDS atomics -- exact, hence independent of the
// order the hardware serves them in -- and converted once.  Only label 0 can hold a NaN (a NaN
// row is labelled 0): a flag makes that sum NaN.  hit: an LDS integer minimum.
__global__ __launch_bounds__(SEG_THREADS) void segments_kernel(const int32_t* __restrict__ label,
                                                               const float* __restrict__ prob, int64_t n, int n_labels,
                                                               const int64_t* __restrict__ window0, int keyword,
                                                               double min_prob, double* __restrict__ sums,
                                                               int32_t* __restrict__ counts, int64_t* __restrict__ hit) {
  __shared__ unsigned long long tot[64];
  __shared__ unsigned int cnt[64];
  __shared__ unsigned int nan0;
  __shared__ int first;
  const int t = threadIdx.x;
  if (t < 64) {
    tot[t] = 0;
    cnt[t] = 0;
  }
  if (t == 0) {
    nan0 = 0;
    first = 0x7fffffff;
  }
  __syncthreads();
  const int64_t s = blockIdx.x;
  int64_t a = window0[s], b = window0[s + 1];
  a = a < 0 ? 0 : a > n ? n : a;
  b = b < a ? a : b > n ? n : b;
  for (int64_t w = a + t; w < b; w += SEG_THREADS) {
    const int l = label[w];
    const float p = prob[w];
    if (l < 0 || l >= n_labels) continue;  // (never written by rows_kernel)
    atomicAdd(&cnt[l], 1u);
    if (p != p) {
      atomicOr(&nan0, 1u);
    } else {
      atomicAdd(&tot[l], (unsigned long long)(p * 536870912.f));  // 2^29: exact
      if (l == keyword && (double)p >= min_prob) atomicMin(&first, (int)(w - a));
    }
  }
  __syncthreads();
  if (t < n_labels) {
    const double v = (double)tot[t] * (1.0 / 536870912.0);
    sums[s * n_labels + t] = (t == 0 && nan0) ? (double)NAN : v;
    counts[s * n_labels + t] = (int32_t)cnt[t];
  }
  if (t == 0) hit[s] = first == 0x7fffffff ? -1 : (int64_t)first;
}

template <int G>
static void launch_rows(const float* logits, int64_t n, int n_labels, int32_t* label, float* prob, hipStream_t st) {
  const int64_t per_block = (ROW_THREADS / 64) * (64 / G);
  hipLaunchKernelGGL(rows_kernel<G>, dim3((unsigned)cdiv(n, per_block)), dim3(ROW_THREADS), 0, st, logits, n,
                     n_labels, label, prob);
}

}  // namespace listen
}  // namespace honk

using namespace honk;

extern "C" int honk_listen_decide_f32(const float* logits, int64_t n, int32_t n_labels, const int64_t* window0_dev,
                                      int64_t segments, int32_t keyword, double min_prob, int32_t* label, float* prob,
                                      double* sums, int32_t* counts, int64_t* hit, void* stream) {
  if (n < 0 || n_labels < 0 || segments < 0)
    return fail(HONK_ERR_ARG, "listen decide: n=%lld n_labels=%d segments=%lld", (long long)n, n_labels,
                (long long)segments);
  if (n_labels < 1 || n_labels > HONK_LISTEN_MAX_LABELS)
    return fail(HONK_ERR_UNSUPPORTED, "listen decide: n_labels=%d outside [1, %d]", n_labels, HONK_LISTEN_MAX_LABELS);
  if (n > HONK_LISTEN_MAX_WINDOWS)
    return fail(HONK_ERR_UNSUPPORTED, "listen decide: n=%lld above %lld windows (the exact sums' limit)", (long long)n,
                (long long)HONK_LISTEN_MAX_WINDOWS);
  if (segments > 0x7fffffff)
    return fail(HONK_ERR_UNSUPPORTED, "listen decide: segments=%lld above one grid", (long long)segments);
  if (n > 0 && (!logits || !label || !prob))
    return fail(HONK_ERR_ARG, "listen decide: null logits / label / prob with n=%lld", (long long)n);
  if (segments > 0 && (!window0_dev || !sums || !counts || !hit))
    return fail(HONK_ERR_ARG, "listen decide: null window0 / sums / counts / hit with segments=%lld",
                (long long)segments);
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    if (n_labels <= 1) listen::launch_rows<1>(logits, n, n_labels, label, prob, st);
    else if (n_labels <= 2) listen::launch_rows<2>(logits, n, n_labels, label, prob, st);
    else if (n_labels <= 4) listen::launch_rows<4>(logits, n, n_labels, label, prob, st);
    else if (n_labels <= 8) listen::launch_rows<8>(logits, n, n_labels, label, prob, st);
    else if (n_labels <= 16) listen::launch_rows<16>(logits, n, n_labels, label, prob, st);
    else if (n_labels <= 32) listen::launch_rows<32>(logits, n, n_labels, label, prob, st);
    else listen::launch_rows<64>(logits, n, n_labels, label, prob, st);
    HONK_LAUNCH_CHECK("listen::rows_kernel");
  }
  if (segments > 0) {
    hipLaunchKernelGGL(listen::segments_kernel, dim3((unsigned)segments), dim3(listen::SEG_THREADS), 0, st, label, prob,
                       n, n_labels, window0_dev, keyword, min_prob, sums, counts, hit);
    HONK_LAUNCH_CHECK("listen::segments_kernel");
  }
  return HONK_OK;
}
