// RPN inference: the post-processing of RPNHead.get_bboxes (mmdet/models/dense_heads/rpn_head.py:79-168,
// anchor_head.py:500-576) between the head's convolutions (dm_conv2d_fwd launches) and the segmented NMS
// (dm_nms_mask_segmented / dm_nms_reduce_segmented).  A SEGMENT is one (image, level); every entry point takes the same
// device table of DM_RPN_SEG_WORDS 64-bit words per segment (dynamask_hip.h, K30).
//
//   dm_rpn_select   per segment, the K candidates of largest dm_sigmoid(logit) in descending order, the lower candidate
//                   index first among equal scores: an exact radix select on the 30 significant bits of the score (three
//                   10-bit digits; a segment is cut into chunks of DM_RPN_SELECT_CHUNK candidates, one workgroup each,
//                   histogram in LDS, merged with integer atomics), a compaction of the selected set in candidate order,
//                   then a rank-by-counting sort of the K survivors (one thread per survivor).  Integer arithmetic only
//                   after the sigmoid: the same bits on every run.
//   dm_rpn_decode   per selected candidate: its anchor (base anchor + grid shift, one fp32 add per coordinate), its four
//                   deltas gathered from the [4 A, H, W] map, delta2bbox_one + clip_box of bbox_decode.h.
//   dm_rpn_merge    per image: the rank of every kept row among the kept rows of all levels (score descending, then
//                   level, then rank within the level), the first nms_post written as [x1, y1, x2, y2, score].
#include "bbox_decode.h"

namespace {

constexpr int RPN_NT = 256;
constexpr int RPN_NW = RPN_NT / DM_WAVE;
constexpr int RPN_CHUNK = DM_RPN_SELECT_CHUNK;
constexpr int RPN_BINS = 1024;
constexpr int RPN_MAX_N = 1 << 20;
constexpr int RPN_MAX_LEVELS = 64;
constexpr unsigned RPN_KEY_ONE = 0x3f800000u;     // the bits of 1.0f: no sigmoid value lies above
constexpr unsigned RPN_KEY_NAN = 0x3f800001u;     // a NaN score sorts first, as in torch.sort(descending=True)
constexpr unsigned RPN_DK_MAX = 0x3fffffffu;

enum { SEG_LOGITS = 0, SEG_DELTAS, SEG_A, SEG_H, SEG_W, SEG_ROWS, SEG_KEY_OFF, SEG_ROW0, SEG_BASE_ROW, SEG_STRIDE_X,
       SEG_STRIDE_Y, SEG_IMAGE };
static_assert(SEG_IMAGE + 1 == DM_RPN_SEG_WORDS, "segment table layout");

// candidate i = (h * W + w) * A + a of an [A, H, W] map: permute(1, 2, 0).reshape(-1)
__device__ __forceinline__ size_t cand_offset(int i, int A, int HW) { return (size_t)(i % A) * HW + (size_t)(i / A); }

// The descending 30-bit key of a sigmoid value in [0, 1] (or NaN): smaller = earlier.
__device__ __forceinline__ unsigned score_dk(float v) {
  const unsigned key = v != v ? RPN_KEY_NAN : min(__float_as_uint(v), RPN_KEY_ONE);
  return RPN_DK_MAX - key;
}

__device__ __forceinline__ int seg_k(int N, int nms_pre) { return nms_pre > 0 ? min(nms_pre, N) : N; }

// Block-wide (RPN_NT threads): the bin holding the k-th smallest entry (1 <= k <= the histogram's total) of a
// RPN_BINS-bin histogram, and k's rank inside that bin.  sh: 8 words of LDS.
__device__ __forceinline__ void find_digit(const unsigned* __restrict__ hist, unsigned k, unsigned& digit, unsigned& k_in,
                                           unsigned* sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned h[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = hist[4 * tid + j];
    s += h[j];
  }
  unsigned incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += sh[w];
  const unsigned excl = incl - s;
  if (excl < k && k <= incl) {          // exactly one thread
    unsigned c = excl;
    int dsel = 4 * tid + 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c + h[j] >= k) {
        dsel = 4 * tid + j;
        break;
      }
      c += h[j];
    }
    sh[4] = (unsigned)dsel;
    sh[5] = k - c;
  }
  __syncthreads();
  digit = sh[4];
  k_in = sh[5];
  __syncthreads();
}

// The first `passes` digits of the K-th smallest key of segment s: prefix (the digits in place) and the rank left.
__device__ __forceinline__ void resolve_prefix(const unsigned* __restrict__ hist_s, int passes, unsigned K, unsigned& prefix,
                                               unsigned& k, unsigned* sh) {
  prefix = 0;
  k = K;
  for (int p = 0; p < passes; ++p) {
    unsigned d;
    find_digit(hist_s + (size_t)p * RPN_BINS, k, d, k, sh);
    prefix |= d << (20 - 10 * p);
  }
}

struct SelArgs {
  const long long* tab;
  int nms_pre, max_chunks;
  unsigned* hist;                 // [S][3][RPN_BINS]
  unsigned* chunk_cnt;            // [S][max_chunks][2]: keys below / equal to the threshold
  unsigned* keys;                 // [total candidates]
  unsigned long long* cand;       // [total rows]: (key << 32) | candidate
  int* idx;
  float* score;
};

// grid = (max_chunks, S).  PASS 0 also computes the keys.
template <int PASS>
__global__ __launch_bounds__(RPN_NT) void rpn_hist_kernel(SelArgs a) {
  __shared__ unsigned lh[RPN_BINS];
  __shared__ unsigned sh[8];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long long* sg = a.tab + (size_t)s * DM_RPN_SEG_WORDS;
  const int A = (int)sg[SEG_A], HW = (int)sg[SEG_H] * (int)sg[SEG_W], N = A * HW;
  const int i0 = blockIdx.x * RPN_CHUNK;
  if (i0 >= N) return;
  unsigned prefix = 0, k = 0;
  if (PASS > 0) resolve_prefix(a.hist + (size_t)s * 3 * RPN_BINS, PASS, (unsigned)seg_k(N, a.nms_pre), prefix, k, sh);
  const unsigned mask = PASS == 0 ? 0u : PASS == 1 ? 0x3ff00000u : 0x3ffffc00u;
  constexpr int shift = 20 - 10 * PASS;
  for (int b = tid; b < RPN_BINS; b += RPN_NT) lh[b] = 0;
  __syncthreads();
  const float* logits = reinterpret_cast<const float*>(sg[SEG_LOGITS]);
  unsigned* keys = a.keys + sg[SEG_KEY_OFF];
  const int i1 = min(i0 + RPN_CHUNK, N);
  for (int i = i0 + tid; i < i1; i += RPN_NT) {
    unsigned dk;
    if (PASS == 0) {
      dk = score_dk(dm_sigmoid(logits[cand_offset(i, A, HW)]));
      keys[i] = dk;
    } else {
      dk = keys[i];
    }
    if ((dk & mask) == prefix) atomicAdd(&lh[(dk >> shift) & (RPN_BINS - 1)], 1u);
  }
  __syncthreads();
  unsigned* gh = a.hist + ((size_t)s * 3 + PASS) * RPN_BINS;
  for (int b = tid; b < RPN_BINS; b += RPN_NT)
    if (lh[b]) atomicAdd(&gh[b], lh[b]);
}

// grid = (max_chunks, S): per chunk, the number of keys below the threshold T and equal to it.
__global__ __launch_bounds__(RPN_NT) void rpn_count_kernel(SelArgs a) {
  __shared__ unsigned sh[8];
  __shared__ unsigned tot[2];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long long* sg = a.tab + (size_t)s * DM_RPN_SEG_WORDS;
  const int N = (int)sg[SEG_A] * (int)sg[SEG_H] * (int)sg[SEG_W];
  const int i0 = blockIdx.x * RPN_CHUNK;
  if (i0 >= N) return;
  unsigned T, k;
  resolve_prefix(a.hist + (size_t)s * 3 * RPN_BINS, 3, (unsigned)seg_k(N, a.nms_pre), T, k, sh);
  if (tid < 2) tot[tid] = 0;
  __syncthreads();
  const unsigned* keys = a.keys + sg[SEG_KEY_OFF];
  const int i1 = min(i0 + RPN_CHUNK, N);
  unsigned lt = 0, eq = 0;
  for (int i = i0 + tid; i < i1; i += RPN_NT) {
    const unsigned dk = keys[i];
    lt += dk < T ? 1u : 0u;
    eq += dk == T ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lt += __shfl_xor(lt, o, 64);
    eq += __shfl_xor(eq, o, 64);
  }
  if ((tid & 63) == 0) {
    atomicAdd(&tot[0], lt);
    atomicAdd(&tot[1], eq);
  }
  __syncthreads();
  if (tid < 2) a.chunk_cnt[((size_t)s * a.max_chunks + blockIdx.x) * 2 + tid] = tot[tid];
}

// grid = (max_chunks, S): the selected set {key < T} + {the first k_eq candidates with key == T}, in candidate order:
// the keys below T at cand[0 .. K - k_eq), the equal ones behind them.
__global__ __launch_bounds__(RPN_NT) void rpn_compact_kernel(SelArgs a) {
  __shared__ unsigned sh[8];
  __shared__ unsigned base[2];
  __shared__ unsigned wcnt[2][RPN_NW];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* sg = a.tab + (size_t)s * DM_RPN_SEG_WORDS;
  const int N = (int)sg[SEG_A] * (int)sg[SEG_H] * (int)sg[SEG_W];
  const int i0 = blockIdx.x * RPN_CHUNK;
  if (i0 >= N) return;
  const unsigned K = (unsigned)seg_k(N, a.nms_pre);
  unsigned T, k_eq;
  resolve_prefix(a.hist + (size_t)s * 3 * RPN_BINS, 3, K, T, k_eq, sh);
  // the chunks before this one
  if (tid < 2) base[tid] = 0;
  __syncthreads();
  {
    unsigned lt = 0, eq = 0;
    const unsigned* cc = a.chunk_cnt + (size_t)s * a.max_chunks * 2;
    for (int c = tid; c < (int)blockIdx.x; c += RPN_NT) {
      lt += cc[2 * c];
      eq += cc[2 * c + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lt += __shfl_xor(lt, o, 64);
      eq += __shfl_xor(eq, o, 64);
    }
    if (lane == 0) {
      atomicAdd(&base[0], lt);
      atomicAdd(&base[1], eq);
    }
  }
  __syncthreads();
  unsigned base_lt = base[0], base_eq = base[1];
  const unsigned n_lt = K - k_eq;
  const unsigned* keys = a.keys + sg[SEG_KEY_OFF];
  unsigned long long* cand = a.cand + sg[SEG_ROW0];
  const int i1 = min(i0 + RPN_CHUNK, N);
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
  for (int t0 = i0; t0 < i1; t0 += RPN_NT) {
    const int i = t0 + tid;
    const unsigned dk = i < i1 ? keys[i] : 0xffffffffu;
    const bool lt = dk < T, eq = dk == T;
    const unsigned long long blt = __ballot(lt), beq = __ballot(eq);
    if (lane == 0) {
      wcnt[0][wave] = (unsigned)__popcll(blt);
      wcnt[1][wave] = (unsigned)__popcll(beq);
    }
    __syncthreads();
    unsigned lt_pos = base_lt + (unsigned)__popcll(blt & below), eq_rank = base_eq + (unsigned)__popcll(beq & below);
    unsigned tot_lt = 0, tot_eq = 0;
#pragma unroll
    for (int w = 0; w < RPN_NW; ++w) {
      const unsigned cl = wcnt[0][w], ce = wcnt[1][w];
      if (w < wave) {
        lt_pos += cl;
        eq_rank += ce;
      }
      tot_lt += cl;
      tot_eq += ce;
    }
    const unsigned long long c = ((unsigned long long)dk << 32) | (unsigned)i;
    if (lt && lt_pos < n_lt) cand[lt_pos] = c;
    if (eq && eq_rank < k_eq) cand[n_lt + eq_rank] = c;
    base_lt += tot_lt;
    base_eq += tot_eq;
    __syncthreads();                      // wcnt is rewritten by the next tile
  }
}

// grid = (ceil(max K / RPN_NT), S): survivor j's rank = the number of survivors with a smaller (key, candidate).
__global__ __launch_bounds__(RPN_NT) void rpn_rank_kernel(SelArgs a) {
  __shared__ unsigned long long tile[RPN_NT];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long long* sg = a.tab + (size_t)s * DM_RPN_SEG_WORDS;
  const int A = (int)sg[SEG_A], HW = (int)sg[SEG_H] * (int)sg[SEG_W], N = A * HW;
  const int K = seg_k(N, a.nms_pre);
  if ((int)blockIdx.x * RPN_NT >= K) return;
  const unsigned long long* cand = a.cand + sg[SEG_ROW0];
  const int j = blockIdx.x * RPN_NT + tid;
  const unsigned long long mine = j < K ? cand[j] : 0ull;
  unsigned rank = 0;
#pragma unroll 1
  for (int t0 = 0; t0 < K; t0 += RPN_NT) {
    tile[tid] = t0 + tid < K ? cand[t0 + tid] : ~0ull;
    __syncthreads();
#pragma unroll 8
    for (int q = 0; q < RPN_NT; ++q) rank += tile[q] < mine ? 1u : 0u;
    __syncthreads();
  }
  if (j >= K) return;
  const int i = (int)(unsigned)(mine & 0xffffffffull);
  const float* logits = reinterpret_cast<const float*>(sg[SEG_LOGITS]);
  a.idx[sg[SEG_ROW0] + rank] = i;
  a.score[sg[SEG_ROW0] + rank] = dm_sigmoid(logits[cand_offset(i, A, HW)]);
}

struct RpnDecodeArgs {
  const long long* tab;
  const int* idx;
  const float* base_anchors;   // [*, 4]
  const float* img_tab;        // [B, 2] (h, w)
  int B;
  float mean[4], std[4];
  float max_ratio;
  float* boxes;                // [total rows, 4]
};

// grid = (ceil(max rows / RPN_NT), S)
__global__ __launch_bounds__(RPN_NT) void rpn_decode_kernel(RpnDecodeArgs a) {
#pragma clang fp contract(off)
  const long long* sg = a.tab + (size_t)blockIdx.y * DM_RPN_SEG_WORDS;
  const int j = blockIdx.x * RPN_NT + threadIdx.x;
  if (j >= (int)sg[SEG_ROWS]) return;
  const int A = (int)sg[SEG_A], H = (int)sg[SEG_H], W = (int)sg[SEG_W], HW = H * W;
  const long long row = sg[SEG_ROW0] + j;
  float* o = a.boxes + (size_t)row * 4;
  const int i = a.idx[row];
  if (i < 0 || i >= A * HW) {             // not a candidate of this segment: no read outside the maps
    o[0] = o[1] = o[2] = o[3] = 0.f;
    return;
  }
  const int an = i % A, p = i / A, w = p % W, h = p / W;
  const float sx = (float)((long long)w * sg[SEG_STRIDE_X]), sy = (float)((long long)h * sg[SEG_STRIDE_Y]);
  const float* ba = a.base_anchors + (size_t)(sg[SEG_BASE_ROW] + an) * 4;
  const float rx1 = ba[0] + sx, ry1 = ba[1] + sy, rx2 = ba[2] + sx, ry2 = ba[3] + sy;
  const float* dl = reinterpret_cast<const float*>(sg[SEG_DELTAS]) + (size_t)(4 * an) * HW + p;
  const float d[4] = {dl[0], dl[HW], dl[2 * (size_t)HW], dl[3 * (size_t)HW]};
  float x1, y1, x2, y2;
  delta2bbox_one(rx1, ry1, rx2, ry2, d, a.mean, a.std, a.max_ratio, x1, y1, x2, y2);
  const int img = min(max((int)sg[SEG_IMAGE], 0), a.B - 1);
  const float ch = a.img_tab[2 * img], cw = a.img_tab[2 * img + 1];
  if (cw > 0.f) clip_box(x1, y1, x2, y2, cw, ch);
  o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
}

// The order-preserving descending key of any float: NaN first, then +inf ... -inf; -0 == +0.
__device__ __forceinline__ unsigned merge_dk(float v) {
  if (v != v) return 0u;
  const unsigned b = v == 0.f ? 0u : __float_as_uint(v);
  const unsigned up = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~up;                           // >= 0x007fffff (+inf): above the NaN key
}

struct MergeArgs {
  const long long* tab;        // segment b * L + l
  int L, nms_post;
  const int* keep;             // [total rows]: segment s's kept rows (within its sorted rows) at keep[row0 ..]
  const int* kept;             // [B * L]
  const float* boxes;          // [total rows, 4]
  const float* score;          // [total rows]
  float* out;                  // [B, nms_post, 5]
  int* counts;                 // [B]
};

// grid = (ceil(max rows of an image / RPN_NT), B): thread t of image b is slot j of the level whose row range holds t.
__global__ __launch_bounds__(RPN_NT) void rpn_merge_kernel(MergeArgs a) {
  __shared__ unsigned long long tile[RPN_NT];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long* tb = a.tab + (size_t)b * a.L * DM_RPN_SEG_WORDS;
  int total_rows = 0, total_kept = 0;
  for (int l = 0; l < a.L; ++l) {
    const int rows = (int)tb[(size_t)l * DM_RPN_SEG_WORDS + SEG_ROWS];
    total_rows += rows;
    total_kept += min(max(a.kept[b * a.L + l], 0), rows);
  }
  if (blockIdx.x == 0 && tid == 0) a.counts[b] = min(total_kept, a.nms_post);
  if ((int)blockIdx.x * RPN_NT >= total_rows) return;
  // this thread's slot
  const int t = blockIdx.x * RPN_NT + tid;
  int lvl = -1, j = 0;
  {
    int cum = 0;
    for (int l = 0; l < a.L; ++l) {
      const int rows = (int)tb[(size_t)l * DM_RPN_SEG_WORDS + SEG_ROWS];
      if (lvl < 0 && t < cum + rows) {
        lvl = l;
        j = t - cum;
      }
      cum += rows;
    }
  }
  bool active = false;
  long long src = 0;
  unsigned long long mine = 0ull;
  if (lvl >= 0) {
    const long long* sg = tb + (size_t)lvl * DM_RPN_SEG_WORDS;
    const int rows = (int)sg[SEG_ROWS];
    if (j < min(max(a.kept[b * a.L + lvl], 0), rows)) {
      const int r = min(max(a.keep[sg[SEG_ROW0] + j], 0), rows - 1);
      src = sg[SEG_ROW0] + r;
      mine = ((unsigned long long)merge_dk(a.score[src]) << 32) | ((unsigned long long)lvl << 20) | (unsigned)j;
      active = true;
    }
  }
  unsigned rank = 0;
  for (int l = 0; l < a.L; ++l) {
    const long long* sg = tb + (size_t)l * DM_RPN_SEG_WORDS;
    const int rows = (int)sg[SEG_ROWS];
    const int km = min(max(a.kept[b * a.L + l], 0), rows);
#pragma unroll 1
    for (int t0 = 0; t0 < km; t0 += RPN_NT) {
      const int e = t0 + tid;
      unsigned long long c = ~0ull;
      if (e < km) {
        const int r = min(max(a.keep[sg[SEG_ROW0] + e], 0), rows - 1);
        c = ((unsigned long long)merge_dk(a.score[sg[SEG_ROW0] + r]) << 32) | ((unsigned long long)l << 20) | (unsigned)e;
      }
      tile[tid] = c;
      __syncthreads();
#pragma unroll 8
      for (int q = 0; q < RPN_NT; ++q) rank += tile[q] < mine ? 1u : 0u;
      __syncthreads();
    }
  }
  if (!active || rank >= (unsigned)a.nms_post) return;
  float* o = a.out + ((size_t)b * a.nms_post + rank) * 5;
  const float* bx = a.boxes + (size_t)src * 4;
  o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3];
  o[4] = a.score[src];
}

struct SelWorkspace {
  size_t cand, hist, chunk_cnt, keys, total;
};

SelWorkspace sel_workspace(int S, int max_n, long long total_n, long long total_rows) {
  SelWorkspace w;
  const size_t chunks = (size_t)dm_ceil_div(max_n, RPN_CHUNK);
  w.cand = 0;
  w.hist = w.cand + (size_t)total_rows * 8;
  w.chunk_cnt = w.hist + (size_t)S * 3 * RPN_BINS * 4;
  w.keys = w.chunk_cnt + (size_t)S * chunks * 2 * 4;
  w.total = w.keys + (size_t)total_n * 4;
  return w;
}

}  // namespace

extern "C" int dm_rpn_select_supported(int num_segments, int max_candidates, long long total_candidates) {
  return num_segments >= 0 && num_segments <= 65535 && max_candidates >= 0 && max_candidates <= RPN_MAX_N &&
                 total_candidates >= 0 && total_candidates <= (long long)num_segments * max_candidates
             ? 1
             : 0;
}

extern "C" long long dm_rpn_select_workspace_bytes(int num_segments, int max_candidates, long long total_candidates,
                                                   long long total_rows) {
  if (!dm_rpn_select_supported(num_segments, max_candidates, total_candidates) || total_rows < 0 ||
      total_rows > total_candidates)
    return -1;
  return (long long)sel_workspace(num_segments, max_candidates, total_candidates, total_rows).total;
}

extern "C" int dm_rpn_select(const long long* seg_tab, int num_segments, int max_candidates, long long total_candidates,
                             long long total_rows, int nms_pre, void* workspace, long long workspace_bytes, int32_t* idx,
                             float* score, dm_stream_t stream) {
  if (num_segments < 0 || max_candidates < 0 || total_candidates < 0 || total_rows < 0) return DM_ERR_INVALID_ARG;
  if (!dm_rpn_select_supported(num_segments, max_candidates, total_candidates)) return DM_ERR_UNSUPPORTED;
  if (total_rows > total_candidates) return DM_ERR_INVALID_ARG;
  if (num_segments == 0 || max_candidates == 0 || total_candidates == 0) return DM_OK;
  const SelWorkspace w = sel_workspace(num_segments, max_candidates, total_candidates, total_rows);
  if (!seg_tab || !workspace || !idx || !score || workspace_bytes < (long long)w.total) return DM_ERR_INVALID_ARG;
  char* ws = static_cast<char*>(workspace);
  SelArgs a;
  a.tab = seg_tab; a.nms_pre = nms_pre; a.max_chunks = dm_ceil_div(max_candidates, RPN_CHUNK);
  a.cand = reinterpret_cast<unsigned long long*>(ws + w.cand);
  a.hist = reinterpret_cast<unsigned*>(ws + w.hist);
  a.chunk_cnt = reinterpret_cast<unsigned*>(ws + w.chunk_cnt);
  a.keys = reinterpret_cast<unsigned*>(ws + w.keys);
  a.idx = idx; a.score = score;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(a.hist, 0, w.chunk_cnt - w.hist, st) != hipSuccess) return DM_ERR_LAUNCH;
  const dim3 grid(a.max_chunks, num_segments);
  DM_LAUNCH(rpn_hist_kernel<0>, grid, dim3(RPN_NT), 0, st, a);
  DM_LAUNCH(rpn_hist_kernel<1>, grid, dim3(RPN_NT), 0, st, a);
  DM_LAUNCH(rpn_hist_kernel<2>, grid, dim3(RPN_NT), 0, st, a);
  DM_LAUNCH(rpn_count_kernel, grid, dim3(RPN_NT), 0, st, a);
  DM_LAUNCH(rpn_compact_kernel, grid, dim3(RPN_NT), 0, st, a);
  const int max_k = nms_pre > 0 ? min(nms_pre, max_candidates) : max_candidates;
  DM_LAUNCH(rpn_rank_kernel, dim3(dm_ceil_div(max_k, RPN_NT), num_segments), dim3(RPN_NT), 0, st, a);
  return dm_check_launch();
}

extern "C" int dm_rpn_decode_supported(int num_segments, int max_rows, int num_images) {
  return num_segments >= 0 && num_segments <= 65535 && max_rows >= 0 && max_rows <= RPN_MAX_N && num_images >= 1 ? 1 : 0;
}

extern "C" int dm_rpn_decode(const long long* seg_tab, int num_segments, int max_rows, const int32_t* idx,
                             const float* base_anchors, const float* img_shapes, int num_images, const float* means,
                             const float* stds, float wh_ratio_clip, float* boxes, dm_stream_t stream) {
  if (num_segments < 0 || max_rows < 0 || !(wh_ratio_clip > 0.f) || !means || !stds) return DM_ERR_INVALID_ARG;
  if (!dm_rpn_decode_supported(num_segments, max_rows, num_images)) return DM_ERR_UNSUPPORTED;
  if (num_segments == 0 || max_rows == 0) return DM_OK;
  if (!seg_tab || !idx || !base_anchors || !img_shapes || !boxes) return DM_ERR_INVALID_ARG;
  RpnDecodeArgs a;
  a.tab = seg_tab; a.idx = idx; a.base_anchors = base_anchors; a.img_tab = img_shapes; a.B = num_images;
  for (int k = 0; k < 4; ++k) { a.mean[k] = means[k]; a.std[k] = stds[k]; }
  a.max_ratio = fabsf(logf(wh_ratio_clip));
  a.boxes = boxes;
  DM_LAUNCH(rpn_decode_kernel, dim3(dm_ceil_div(max_rows, RPN_NT), num_segments), dim3(RPN_NT), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}

extern "C" int dm_rpn_merge_supported(int num_images, int num_levels, int max_rows, int nms_post) {
  return num_images >= 0 && num_images <= 65535 && num_levels >= 1 && num_levels <= RPN_MAX_LEVELS && max_rows >= 0 &&
                 max_rows <= RPN_MAX_N && nms_post >= 1
             ? 1
             : 0;
}

extern "C" int dm_rpn_merge(const long long* seg_tab, int num_images, int num_levels, int max_rows, const int32_t* keep,
                            const int32_t* kept, const float* boxes, const float* score, int nms_post, float* out,
                            int32_t* counts, dm_stream_t stream) {
  if (num_images < 0 || num_levels < 0 || max_rows < 0) return DM_ERR_INVALID_ARG;
  if (!dm_rpn_merge_supported(num_images, num_levels, max_rows, nms_post)) return DM_ERR_UNSUPPORTED;
  if (num_images == 0) return DM_OK;
  if (!seg_tab || !kept || !out || !counts || (max_rows > 0 && (!keep || !boxes || !score))) return DM_ERR_INVALID_ARG;
  MergeArgs a;
  a.tab = seg_tab; a.L = num_levels; a.nms_post = nms_post; a.keep = keep; a.kept = kept; a.boxes = boxes; a.score = score;
  a.out = out; a.counts = counts;
  const long long img_rows = (long long)max_rows * num_levels;
  DM_LAUNCH(rpn_merge_kernel, dim3(max(1, dm_ceil_div(img_rows, RPN_NT)), num_images), dim3(RPN_NT), 0,
            (hipStream_t)stream, a);
  return dm_check_launch();
}
