// K5/K6/K16: dense stride-1 "same" convolution (1x1 / 3x3) and deconv 2x2/s2 as an
// implicit GEMM on the fp32-input MFMA units of gfx950 (v_mfma_f32_32x32x2_f32:
// exact fp32 fma chain, 1e-4 parity with the fp32 reference by construction).
//
// GEMM view (per launch):   Out[co, q] = bias[co] + sum_k  Wq[k, co] * X[k, q]
//   rows   co : output channels (MFMA "A" operand = packed weights, M side)
//   cols   q  : FLAT pixel index over the whole batch, q = n*H*W + y*W + x
//               (MFMA "B" operand = the im2col of the input, N side).  Flat
//               columns: no padding waste for 14x14 RoI maps (196 px), one kernel
//               for RoI tensors and whole FPN maps alike.
//   k         : (tap, input channel); the channel concatenation of up to 4
//               source tensors is walked in the K loop (torch.cat never
//               materialises).
// The 32x32 MFMA D layout puts the pixel on the lane, so every accumulator
// register stores 32 consecutive pixels of one output channel: 128-B coalesced
// NCHW stores.
//
// K ordering is ours to choose, so input channels are handled in QUADS: packed
// weights are [tap][channel quad][cout][4] and the LDS images are
//   A: [tap][quad][TM couts][4]      B: [quad][plane position][4]
// so ONE ds_read_b128 per operand feeds FOUR k-steps: MFMA j of a quad pair
// uses k = j (lanes 0-31, even quad) and k = 4+j (lanes 32-63, odd quad).
// Consecutive lanes read consecutive 16-B slots: conflict-free.
//
// Pipeline per workgroup (256 threads, 4 waves, 2x2 32x32 blocks per wave at
// the 128x128 tile): the NEXT chunk's global loads are issued into registers
// before the MFMAs of the current chunk and written to LDS after them
// (issue-early / write-late), so L2 latency hides under 144 MFMAs per wave.
// The builds without an A image (conv_direct_a) have a K loop of their own:
// a ring of weight-fragment sets that runs on through the chunks, and the next
// chunk's staging loads dealt over the current chunk's steps, unpredicated.
#include <type_traits>

#include "common.h"

namespace {

// dm_conv2d_plan's / dm_conv2d_group_plan's recorder (host side): conv_emit writes one record per problem of each launch it
// would make, and nothing is launched.
// A record is DM_CONV_PLAN_INTS ints in the order the header documents.
struct ConvPlan {
  int cap;             // records the caller's array holds: DM_CONV_PLAN_MAX_LAUNCHES (lone) or DM_CONV_GROUP_PLAN_MAX
  int count = 0;
  int rec[DM_CONV_GROUP_PLAN_MAX][DM_CONV_PLAN_INTS];
  int copy_to(int* records) const {      // -> the number of records
    for (int l = 0; l < count; ++l)
      for (int i = 0; i < DM_CONV_PLAN_INTS; ++i) records[l * DM_CONV_PLAN_INTS + i] = rec[l][i];
    return count;
  }
};
static_assert(DM_CONV_GROUP_PLAN_MAX >= DM_CONV_PLAN_MAX_LAUNCHES, "one array holds either plan");

struct ConvArgs {
  const float* src[DM_MAX_SOURCES];
  int src_c[DM_MAX_SOURCES];
  long long src_bs[DM_MAX_SOURCES];  // batch stride of each source, in floats
  int num_srcs;
  int NB, H, W, HW, Q;
  const float* wq;   // [taps][KQ][CoutP][4]
  const float* bias;
  int KQ, Cout, CoutP;
  int relu;   // flags: bit0 = ReLU, bit1 = accumulate into out
  float* out;
  int out_ch_total, out_ch_offset;
  int Wp, plane;  // 3x3: W+2, Rmax*Wp ; 1x1: unused, TN
  int MT;         // number of cout tiles
  int q_begin = 0;  // first flat pixel of this launch (Q is its end): a launch may cover a pixel range
  int shuffle;    // deconv 2x2/s2 epilogue: packed cout = phase*shuffle + co, stored at (2y+dy, 2x+dx)
  const float* mask = nullptr;   // same layout as out: outputs whose mask value is not > 0 are stored as 0 (a ReLU adjoint)
  int off32 = 0;     // every source spans < 4 GB: a pixel's offset inside a source fits 32 bits (the 1x1 builds' branch-free staging)
  // split-K (round 4; launches of few workgroups -- the <= 100-RoI inference calls): blockIdx.y = split, which walks
  // kchunks chunks of the K loop from chunk split * kchunks and stores its bare sums to ws + split * ws_stride
  // ([NB][Cout][HW]); conv_splitk_reduce_kernel adds the splits in index order and applies bias / accumulate / ReLU / mask
  float* ws = nullptr;
  long long ws_floats = 0, ws_stride = 0;
  int ksplit = 1, kchunks = 0;
  int want_split = 0;        // host side: the launcher's choice of splits for this launch (0: launch_conv_mp decides)
  // POST builds (dm_conv2d_post_add_fwd): same layout as out, added AFTER the activation; may be out itself
  const float* addend = nullptr;
  // POST == 2 builds (K31, dm_conv2d_up_add_fwd): addend is a dense [NB, Cout, up_Hs, up_Ws] map of its own, read at
  // (up_iy[y], up_ix[x]) -- device tables of H and W entries; up_plane = up_Hs * up_Ws, its channel stride
  const int* up_iy = nullptr;
  const int* up_ix = nullptr;
  int up_Ws = 0, up_plane = 0;
  ConvPlan* plan = nullptr;  // host side, null in every product call: record the launch instead of making it (dm_conv2d_plan)
};

// CK input channels per chunk (multiple of 8); MAXPOS = plane positions per thread (3x3)
// TAIL (0 or 4): output channels TM .. TM+3 are computed with v_mfma_f32_4x4x1 (16 blocks of
// 4 x 4: the 4 lanes of a block hold the 4 tail couts as A and 4 pixels as B, so a lane
// accumulates the 4 tail couts of ITS pixel) from the same B fragments -- the 36-cout offset
// convs of the DCN layers then cost 32 + 4 rows of MFMA work instead of 64.
// The 3x3 128 x 128 build with one plane position per thread is held to 168 VGPRs (5 dwords of
// scratch): three workgroups per CU instead of two hide each other's barriers better
// (14 x 14, 3 full rounds: 0.916 -> 0.876 ms; 752 RoIs: 135 TFLOP/s; 150 VGPRs and no scratch since its weight fragments
// come from the packed tensor: conv_direct_a below).  The 1x1 builds with 32-channel
// chunks spill 35-55 dwords at 168 and lose a third of their rate; with 16-channel chunks (half the
// prefetch registers) they fit without scratch, and three per CU beats the longer chunk: the DCN
// column-gradient GEMMs 1.56 -> 1.20, 0.94 -> 0.78, 0.75 -> 0.67 ms, fusion 130->64 @56^2 0.56 -> 0.45 ms.
// The kernel body takes its place in the grid as arguments (bx of gx workgroups, split by): conv_igemm_kernel passes
// blockIdx / gridDim, conv_igemm_group_kernel (several independent convolutions in one launch) a range of its grid.
//
// PREC (round 7, opt-in: flag bit 4 of dm_conv2d_fwd / dm_conv2d_fwd_ws / dm_conv1x1_group_fwd, inference only): the
// bf16x3 split on the bf16 matrix cores.  An fp32 value is cut into three bf16 planes with round-to-nearest,
// x = hi + mid + lo (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 24 significant bits), and a product is
// the six largest cross terms lo*hi + mid*mid + hi*lo + mid*hi + hi*mid + hi*hi -- six v_mfma_f32_32x32x16_bf16 per 16
// channels, issued in that fixed order (smallest first), accumulated in fp32: the five correction terms in an accumulator
// of their own, added to hi*hi's once at the end (their roundings then are ~2^-8 of the main sum's).  The dropped terms are below 2^-24
// relative: sums differ from the exact kernel's in rounding only.  16 channels x 32 cycles per bf16 MFMA against 2 x 64
// per v_mfma_f32_32x32x2_f32: 16 x 64 / (6 x 32 x 2) = 2.7 x the fp32 matrix rate.  K is walked in chunks of 16 channels;
// a "word" (16 bytes) holds 8 consecutive channels of one (cout | pixel) as bf16, and the six words of a chunk are
// (channels 0-7 | 8-15) x (hi, mid, lo).  Weights are split once, by pack_weight_bf16x3_kernel (sources padded to 16
// channels); activations when a thread commits its prefetched floats to LDS (once per staged value: split at the read,
// a 3x3 tile would split each value nine times, once per tap, in the MFMA loop).  When hi is not finite, mid = lo = 0,
// so an Inf or NaN operand makes the same outputs non-finite as in the exact kernel (the pattern is kept, not the
// value: Inf times a zero mid or lo plane of the other operand is NaN where the exact kernel has +-Inf).  Only 64-cout x 128-pixel tiles and no TAIL rows are built: a
// 36-cout launch (the DCN offset convolutions) runs as one 64-cout tile, its tail couts on the bf16 MFMA like the rest;
// launches the split build does not cover (3x3 maps wider than ~16 pixels) return DM_ERR_UNSUPPORTED, and the host's
// routing table (ops.BF16X3_ROUTES) keeps the shapes where the split is not faster on the exact kernel.
typedef __bf16 dm_bf16x8 __attribute__((ext_vector_type(8)));

// x -> (hi, mid, lo), round-to-nearest-even; fp32 subnormal residuals are kept (bf16 has fp32's exponent range, and the
// build keeps fp32 denormals), a non-finite hi gets mid = lo = 0
__device__ __forceinline__ void dm_split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float hf = (float)h;
  if (__builtin_isfinite(hf)) {
    const float r1 = x - hf;          // exact: hf is x rounded to 8 significant bits
    m = (__bf16)r1;
    l = (__bf16)(r1 - (float)m);      // exact likewise
  } else {
    m = (__bf16)0.f;
    l = (__bf16)0.f;
  }
}

// 8 floats -> their hi, mid and lo words (8 bf16 each)
__device__ __forceinline__ void dm_split8x3(const dm_f32x4& q0, const dm_f32x4& q1, dm_f32x4 (&out)[3]) {
  dm_bf16x8 w[3];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 h, m, l;
    dm_split3(e < 4 ? q0[e] : q1[e - 4], h, m, l);
    w[0][e] = h;
    w[1][e] = m;
    w[2][e] = l;
  }
#pragma unroll
  for (int p = 0; p < 3; ++p) out[p] = __builtin_bit_cast(dm_f32x4, w[p]);
}

// Builds that read their weight (A) fragments straight from the packed tensor: the exact fp32 128 x 128 builds (four waves
// of 2 x 2 MFMA blocks, no tail rows) of the 3x3 kernel at every MAXPOS and of the 1x1 kernel with 16-channel chunks, POST
// twin and grouped launches included.  A wave's fragment of a step is one 16-byte load per lane and 32-row block from
// [tap][quad][cout][4] -- 512 contiguous bytes per half-wave, L2 hits: every workgroup of a launch walks the same weights
// -- into the registers the MFMAs read, two steps ahead (the ring of the K loop below).  Such a build has no A image in LDS
// (ldsB starts at 0) and none of its traffic: per wave and 8-channel chunk of the 3x3 build 9 global loads, 9 ds_write_b128
// and 18 ds_read_b128 become 18 buffer loads.  A compile-time property of the build: the launchers size the LDS with it,
// nothing else knows it. DM_CONV_DIRECT_A (bit 0: the 3x3 builds, bit 1: the 1x1 builds) says which of them take the path.
// The 1x1 builds are OFF: measured against the LDS image (profiles/conv_direct_weights.txt) the fusion GEMM 514 -> 256 @14
// lost 6 % in every pass (0.286 / 0.293 -> 0.303 / 0.310 ms), and with the ring loop below it still loses 4 % (0.290 /
// 0.286 / 0.286 -> 0.301 / 0.295 / 0.298 ms, profiles/conv_fragment_ring.txt): with two steps per chunk the next chunk's
// staging loads have to land inside the chunk they are issued in, whatever the waits count.  The 3x3 builds gained in every
// pass (conv 256 -> 256 @14: 1.041 / 1.056 -> 1.011 / 1.029 ms).  -DDM_CONV_DIRECT_A=n: A/B libraries.
#ifndef DM_CONV_DIRECT_A
#define DM_CONV_DIRECT_A 1
#endif
template <int KS, int WGM, int WGN, int WM, int WN, int CK, int TAIL, int PREC>
constexpr bool conv_direct_a() {
  return PREC == 0 && TAIL == 0 && WGM == 2 && WGN == 2 && WM == 2 && WN == 2 &&
         ((KS == 3 && CK == 8 && (DM_CONV_DIRECT_A & 1)) || (KS == 1 && CK == 16 && (DM_CONV_DIRECT_A & 2)));
}

// POST (K26, dm_conv2d_post_add_fwd): the epilogue stores addend + act(conv + bias) -- the addend joins after the
// activation, where the accumulate flag adds before it; everything in front of the store is the POST = 0 build's.
template <int KS, int WGM, int WGN, int WM, int WN, int CK, int MAXPOS, int TAIL = 0, int PREC = 0, int POST = 0>
__device__ __forceinline__ void conv_igemm_body(const ConvArgs& a, const int bx, const int gx, const int by) {
  static_assert(TAIL == 0 || (TAIL == 4 && WGM == 1), "tail rows need a single cout tile");
  static_assert(PREC == 0 || (PREC == 1 && CK == 16 && TAIL == 0 && WM == 1 && WN == 2 && WGM == 2 && WGN == 2),
                "the bf16x3 build: 64 x 128 tiles, 16-channel chunks, no tail rows");
  static_assert(POST == 0 || (KS == 1 && TAIL == 0 && PREC == 0), "the post-activation addend: exact fp32 1x1 builds");
  constexpr int TM = WGM * WM * 32;
  constexpr int TMA = TM + TAIL;              // rows of the LDS A image
  constexpr int TN = WGN * WN * 32;
  constexpr int NT = WGM * WGN * 64;
  constexpr int TAPS = KS * KS;
  constexpr int NQ = CK / 4;                      // channel quads per chunk (what a thread prefetches of a pixel)
  constexpr int NWC = PREC ? 6 : NQ;              // 16-byte words per chunk and (cout | pixel) in LDS and in the packed weights
  constexpr bool DIRECT = conv_direct_a<KS, WGM, WGN, WM, WN, CK, TAIL, PREC>();      // A fragments from the packed tensor
  constexpr int A_F4 = DIRECT ? 0 : TAPS * NWC * TMA;      // float4 slots of the A chunk in LDS
  constexpr int A_PER_T = (A_F4 + NT - 1) / NT;
  constexpr int AREG = A_PER_T ? A_PER_T : 1;
  constexpr int B1_PER_T = (NQ * TN + NT - 1) / NT;   // 1x1: float4 slots per thread
  constexpr int BREG = (KS == 3) ? MAXPOS * NQ : B1_PER_T;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  dm_f32x4* ldsA = reinterpret_cast<dm_f32x4*>(lds);                 // [TAPS][NQ][TM]
  dm_f32x4* ldsB = reinterpret_cast<dm_f32x4*>(lds) + A_F4;          // [NWC][plane]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = wave / WGN;
  const int wave_n = wave % WGN;
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own
  // L2), so the MT cout tiles of one pixel tile -- which read the same input -- are placed
  // 8 apart in launch order: same XCD, back to back.  The ragged tail keeps the plain order.
  int m_tile, n_tile;
  {
    const int b = bx, grp = 8 * a.MT;
    const int full = (gx / grp) * grp;
    if (b < full) {
      const int g = b / grp, r = b - g * grp;
      m_tile = r / 8;
      n_tile = g * 8 + (r & 7);
    } else {
      const int r = b - full;
      m_tile = r % a.MT;
      n_tile = full / a.MT + r / a.MT;
    }
  }
  const int m0 = m_tile * TM;
  const int q0 = a.q_begin + n_tile * TN;
  const int HW = a.HW, W = a.W, H = a.H;
  const int plane = a.plane;
  int k_skip = 0, k_left = 0x7fffffff;         // split-K: chunks to pass over, chunks to walk
  // the epilogue's destination and modes (locals: writing to the argument struct would copy all of it to scratch)
  float* e_out = a.out;
  const float* e_bias = a.bias;
  const float* e_mask = a.mask;
  int e_relu = a.relu, e_oct = a.out_ch_total, e_oco = a.out_ch_offset;
  if (a.ksplit > 1) {
    const int sp = by;
    e_out = a.ws + (size_t)sp * a.ws_stride;
    e_bias = nullptr; e_mask = nullptr; e_relu = 0;
    e_oct = a.Cout; e_oco = 0;
    k_skip = sp * a.kchunks; k_left = a.kchunks;
  }

  // ---- tile geometry (uniform) -------------------------------------------
  const int qlast = min(q0 + TN, a.Q) - 1;
  const int n0 = q0 / HW;
  const int n1 = qlast / HW;
  const int y00 = (q0 - n0 * HW) / W;
  const int y1l = (qlast - n1 * HW) / W;
  const int rows0 = (n1 > n0) ? (H - y00) : (y1l - y00 + 1);
  const int Wp = a.Wp;

  // ---- per-lane column bookkeeping ----------------------------------------
  int lane_base[WN];   // LDS float4 index of tap (0,0) of this lane's pixel (+ odd-quad offset)
  int col_n[WN], col_p[WN];
  bool col_ok[WN];
#pragma unroll
  for (int wn = 0; wn < WN; ++wn) {
    const int j = (wave_n * WN + wn) * 32 + l31;
    int q = q0 + j;
    col_ok[wn] = q < a.Q;
    q = min(q, a.Q - 1);
    const int n = q / HW;
    const int p = q - n * HW;
    col_n[wn] = n;
    col_p[wn] = p;
    if (KS == 3) {
      const int y = p / W;
      const int x = p - y * W;
      const int seg = n - n0;
      const int r = (seg == 0) ? (y - y00 + 1) : (rows0 + 2) + (seg - 1) * (H + 2) + (y + 1);
      lane_base[wn] = (r - 1) * Wp + x + (PREC ? 3 * hi : hi) * plane;      // (PREC: lane half = channels 8 hi .. = words 3 hi ..)
    } else {
      lane_base[wn] = j + (PREC ? 3 * hi : hi) * plane;
    }
  }

  // ---- B staging assignment (fixed for the tile) ---------------------------
  //  3x3: thread -> up to MAXPOS plane positions (all CK channels of each)
  //  1x1: thread -> column j = tid % TN, quads (tid / TN) + i * (NT / TN)
  int st_pix[(KS == 3) ? MAXPOS : 1], st_n[(KS == 3) ? MAXPOS : 1];
  if (KS == 3) {
    const int Rused = (n1 == n0) ? (rows0 + 2) : (rows0 + 2) + (n1 - n0 - 1) * (H + 2) + (y1l + 3);
#pragma unroll
    for (int k = 0; k < MAXPOS; ++k) {
      const int pos = tid + k * NT;
      st_n[k] = -1;
      st_pix[k] = 0;
      if (pos < plane) {
        const int r = pos / Wp;
        const int c = pos - r * Wp;
        int seg, y;
        if (r < rows0 + 2) {
          seg = 0;
          y = y00 - 1 + r;
        } else {
          const int rr = r - (rows0 + 2);
          seg = 1 + rr / (H + 2);
          y = rr % (H + 2) - 1;
        }
        const int n = n0 + seg;
        if (r < Rused && n < a.NB && y >= 0 && y < H && c >= 1 && c <= W) {
          st_n[k] = n;
          st_pix[k] = y * W + (c - 1);
        }
      }
    }
  } else {
    int q = q0 + (tid % TN);
    const bool ok = q < a.Q;
    q = min(q, a.Q - 1);
    const int n = q / HW;
    st_pix[0] = q - n * HW;
    st_n[0] = ok ? n : -1;
  }

  dm_f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  constexpr int WMX = PREC ? WM : 1, WNX = PREC ? WN : 1;
  dm_f32x16 accx[WMX][WNX];   // PREC: the correction terms' accumulators
#pragma unroll
  for (int i = 0; i < WMX; ++i)
#pragma unroll
    for (int j = 0; j < WNX; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) accx[i][j][r] = 0.f;
  dm_f32x4 acct[WN];      // tail couts TM .. TM+3 of this lane's pixel (lanes >= 32: the other K half)
#pragma unroll
  for (int j = 0; j < WN; ++j) acct[j] = dm_f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- chunk iterator over (source, channel offset) ------------------------
  int cs = 0, cc0 = 0, ckq = 0;   // current source, channel offset in it, global quad index of the chunk
  int curC = a.src_c[0];          // channels of the current source (kept in a register: a.src_c[cs] is a scalar load from the
                                  // argument block, and its s_waitcnt lgkmcnt(0) in the K loop also waits for the LDS)
  auto chunk_valid = [&]() { return cs < a.num_srcs && k_left > 0; };
  auto chunk_advance = [&]() {
    const int ckv = min(CK, curC - cc0);
    ckq += PREC ? NWC : ((ckv + 7) / 8) * 2;      // (PREC: every source is padded to whole 16-channel chunks)
    cc0 += CK;
    if (cc0 >= curC) {
      cs++;
      cc0 = 0;
      curC = cs < a.num_srcs ? a.src_c[cs] : 0;
    }
  };

  dm_f32x4 ra[AREG];
  dm_f32x4 rb[BREG];
  unsigned a_off[AREG];          // float offset of A slot i inside a chunk's weights (fixed per thread)
#pragma unroll
  for (int i = 0; i < A_PER_T; ++i) {
    const int idx = tid + i * NT;
    const int m = idx % TMA, tq = idx / TMA;
    a_off[i] = (unsigned)((((size_t)(tq / NWC) * a.KQ + tq % NWC) * a.CoutP + min(m0 + m, a.CoutP - 1)) * 4);      // (rows past CoutP: the last row)
  }
  constexpr int NPOS = (KS == 3) ? MAXPOS : 1;
  size_t b_off[NPOS];               // float offset of this thread's pixel(s) inside the current source
  int b_src = -1;
  unsigned b_off32 = 0;             // 1x1 fast path: the same offset in 32 bits
  const float* b_srcp = nullptr;    // 1x1 fast path: base of the current source

  // DIRECT: the A fragment of step (tap, quad pair g) of the chunk whose first quad is cq -- lanes 0-31 quad 2 g, lanes 32-63
  // quad 2 g + 1 of cout rows (wave_m WM + i) 32 + l31, the lane layout of the LDS image.  Through a buffer descriptor: the
  // lane's part of the address is one 32-bit register fixed for the whole K loop (rows past CoutP: the last row again, never
  // stored), the chunk / tap / quad-pair part is scalar.  (Flat 64-bit addresses keep a register pair per tap alive through
  // the loop: deform_conv_c256_kernel.)  The descriptor ends with the packed tensor (the launcher keeps it below 2 GB).
  constexpr int NGD = NQ / 2;                       // quad pairs per chunk = MFMA steps per tap
  const __amdgpu_buffer_rsrc_t wsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wq), 0, DIRECT ? TAPS * a.KQ * a.CoutP * 16 : 0, 0x00020000);
  const int a_quad = a.CoutP * 16, a_tap = a.KQ * a_quad;      // bytes per channel quad / per tap of the packed weights
  unsigned a_lane[WM];                              // bytes
#pragma unroll
  for (int i = 0; i < WM; ++i) a_lane[i] = 16u * (unsigned)(hi * a.CoutP + min(m0 + (wave_m * WM + i) * 32 + l31, a.CoutP - 1));
  // ng: the chunk's quad pairs with live channels.  A dead quad pair (a 1x1 chunk of at most 8 channels) is not in the
  // packed tensor at all: its step loads the chunk's last live pair again, and no MFMA reads it.
  auto load_a = [&](int cq, int ng, int st, dm_f32x4* av) {
    const int tap = st / NGD, g = min(st - tap * NGD, ng - 1);
    const int so = tap * a_tap + (cq + 2 * g) * a_quad;
#pragma unroll
    for (int i = 0; i < WM; ++i) av[i] = __builtin_bit_cast(dm_f32x4, __builtin_amdgcn_raw_buffer_load_b128(wsrc, a_lane[i], so, 0));
  };

  // issue the global loads of the chunk at (cs, cc0, ckq) into registers
  auto prefetch = [&]() {
    const int ckv = min(CK, curC - cc0);
    const int nq = PREC ? NWC : ((ckv + 7) / 8) * 2;    // quads (words) of this chunk present in the packed weights
    // the chunk's part of an address is uniform (ckq, cc0); the thread's part is fixed for the K loop
    // (per source for B) and kept in a register: no 64-bit multiplies per load next to the MFMAs
    const float* abase = a.wq + (size_t)ckq * a.CoutP * 4;
    if (KS == 1 && (A_F4 % NT == 0 || PREC) && NQ * TN % NT == 0 && a.off32 && ckv == CK) {
      // Full chunk of a 1x1 build: nothing is predicated.  (The general path below guards every dword -- pixel inside the
      // matrix, channel inside the source, quad inside the chunk -- with an exec-mask branch and a 64-bit vector address:
      // ~150 instructions per 16 MFMAs in the 64-cout build, 4.8 VALU + 5.6 SALU per MFMA on the 576 -> 64 GEMM
      // (profiles/r03_sq_pmc.txt) against 1.65 + 0.97 in the 3x3 build.)  A pixel past the matrix stages the pixel the
      // thread was clamped to -- its output column is never stored; rows past CoutP repeat the last row.  Addresses are a
      // uniform row base (SALU) plus the thread's 32-bit pixel offset.
#pragma unroll
      for (int i = 0; i < A_PER_T; ++i)
        if (A_F4 % NT == 0 || tid + i * NT < A_F4) ra[i] = *reinterpret_cast<const dm_f32x4*>(abase + a_off[i]);   // (PREC: wave-uniform)
      if (b_src != cs) {
        b_off32 = (unsigned)((size_t)max(st_n[0], 0) * (size_t)a.src_bs[cs] + st_pix[0]);
        b_srcp = a.src[cs];
        b_src = cs;
        b_off[0] = b_off32;
      }
      const float* rp = b_srcp + (size_t)cc0 * HW;
      const int qw = (TN % 64 == 0) ? __builtin_amdgcn_readfirstlane(tid / TN) : tid / TN;      // (uniform per wave from 64 columns on)
#pragma unroll
      for (int i = 0; i < B1_PER_T; ++i) {
        // (PREC: a thread stages the two quads of one 8-channel half -- commit splits them into its three words)
        const float* rq = rp + (size_t)((PREC ? qw * 2 + i : qw + i * (NT / TN)) * 4) * HW;
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[i][e] = rq[(size_t)e * HW + b_off32];
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int idx = tid + i * NT;
      dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < A_F4) {
        const int m = idx % TMA;
        const int qd = (idx / TMA) % NWC;
        if (qd < nq && m0 + m < a.CoutP) v = *reinterpret_cast<const dm_f32x4*>(abase + a_off[i]);
      }
      ra[i] = v;
    }
    if (b_src != cs) {
      const size_t bs = (size_t)a.src_bs[cs];
#pragma unroll
      for (int k = 0; k < NPOS; ++k) b_off[k] = (size_t)max(st_n[k], 0) * bs + st_pix[k];
      b_src = cs;
    }
    const float* sp = a.src[cs] + (size_t)cc0 * HW;
    if (KS == 3 && ckv == CK) {
      // full chunk: ONE guard per plane position (its pixel exists or it is padding) instead of one per dword
#pragma unroll
      for (int k = 0; k < MAXPOS; ++k) {
        const float* gp = sp + b_off[k];
        if (st_n[k] >= 0) {
#pragma unroll
          for (int qd = 0; qd < NQ; ++qd)
#pragma unroll
            for (int e = 0; e < 4; ++e) rb[k * NQ + qd][e] = gp[(size_t)(qd * 4 + e) * HW];
        } else {
#pragma unroll
          for (int qd = 0; qd < NQ; ++qd) rb[k * NQ + qd] = dm_f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    } else if (KS == 3) {
#pragma unroll
      for (int k = 0; k < MAXPOS; ++k) {
        const bool ok = st_n[k] >= 0;
        const float* gp = sp + b_off[k];
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd) {
          dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int ci = qd * 4 + e;
            if (ok && ci < ckv) v[e] = gp[(size_t)ci * HW];
          }
          rb[k * NQ + qd] = v;
        }
      }
    } else {
      const bool ok = st_n[0] >= 0;
      const float* gp = sp + b_off[0];
#pragma unroll
      for (int i = 0; i < B1_PER_T; ++i) {
        const int qd = PREC ? (tid / TN) * 2 + i : tid / TN + i * (NT / TN);
        dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ci = qd * 4 + e;
          if (ok && qd < NQ && ci < ckv) v[e] = gp[(size_t)ci * HW];
        }
        rb[i] = v;
      }
    }
  };

  // DIRECT: the chunk whose B values are in flight to rb (the staging cursor): its first channel in its source and its live
  // channels.  The staging loads of these builds are never predicated: a padding position reads pixel 0 of image 0, a channel
  // past the source the source's last one, and commit() SELECTS the zero (a select, not a product: the value read may be Inf).
  const float* st_base = nullptr;
  int st_ckv = CK;
  const int st_qw = (KS == 1 && TN % 64 == 0) ? __builtin_amdgcn_readfirstlane(tid / TN) : tid / TN;      // 1x1: the thread's first quad
  auto st_channel = [&](int i, int e) {      // channel inside the chunk of element e of rb[i]
    return ((KS == 3 ? i % NQ : st_qw + i * (NT / TN)) * 4 + e);
  };

  auto commit = [&]() {   // registers -> LDS
    if constexpr (DIRECT) {
#pragma unroll
      for (int i = 0; i < BREG; ++i) {
        const int lim = st_n[KS == 3 ? i / NQ : 0] >= 0 ? st_ckv : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[i][e] = st_channel(i, e) < lim ? rb[i][e] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int idx = tid + i * NT;
      if (idx < A_F4) ldsA[idx] = ra[i];
    }
    if (PREC) {
      // fp32 -> three bf16 words per 8-channel half: [channels 0-7: hi, mid, lo][channels 8-15: hi, mid, lo]
      if (KS == 3) {
#pragma unroll
        for (int k = 0; k < MAXPOS; ++k) {
          const int pos = tid + k * NT;
          if (pos < plane) {
#pragma unroll
            for (int h8 = 0; h8 < 2; ++h8) {
              dm_f32x4 wd[3];
              dm_split8x3(rb[k * NQ + 2 * h8], rb[k * NQ + 2 * h8 + 1], wd);
#pragma unroll
              for (int p_ = 0; p_ < 3; ++p_) ldsB[(3 * h8 + p_) * plane + pos] = wd[p_];
            }
          }
        }
      } else {
        static_assert(!PREC || KS == 3 || (B1_PER_T == 2 && NT / TN == 2), "1x1 bf16x3 build: two quads (one half) per thread");
        const int h8 = tid / TN;
        dm_f32x4 wd[3];
        dm_split8x3(rb[0], rb[B1_PER_T > 1 ? 1 : 0], wd);
#pragma unroll
        for (int p_ = 0; p_ < 3; ++p_) ldsB[(3 * h8 + p_) * plane + (tid % TN)] = wd[p_];
      }
    } else if (KS == 3) {
#pragma unroll
      for (int k = 0; k < MAXPOS; ++k) {
        const int pos = tid + k * NT;
        if (pos < plane) {
#pragma unroll
          for (int qd = 0; qd < NQ; ++qd) ldsB[qd * plane + pos] = rb[k * NQ + qd];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < B1_PER_T; ++i) {
        const int qd = tid / TN + i * (NT / TN);
        if (qd < NQ) ldsB[qd * plane + (tid % TN)] = rb[i];
      }
    }
  };

  for (; k_skip > 0 && cs < a.num_srcs; --k_skip) chunk_advance();      // (split-K: this split's first chunk)
  if constexpr (DIRECT) {
    // ---- the K loop of the builds without an A image --------------------------------------------------------------------
    // One stream of steps runs on through the chunks (STEPS per chunk; a dead quad pair of a ragged 1x1 chunk keeps its
    // place in the stream, its MFMAs are skipped).  Issued under step s: the ds_reads of step s + 1's B fragments, the A
    // fragment load of step s + D into the ring's free set, the next chunk's staging loads of this step (LPS dwords of the
    // chunk's NLD) -- one by one between the step's MFMAs on the ring's oldest set.  Loads return in order, so the wait in
    // front of step s's MFMAs is for a fragment with the younger fragment loads and staging loads behind it, which stay in
    // flight -- and the compiler can count them: nothing in the loop is predicated.  (Steps 2 .. 8 of a chunk, in the ISA;
    // step 0's wait is vmcnt(2) behind step 2's fragment load, which lands step 1's fragment a step early, and step 1 has
    // none.)  Where there is no next chunk the cursors stay on the current one (its values are loaded once more and
    // dropped), so the last chunk is not a special case. Split-K starts the stream at its first chunk; a source change only
    // moves the cursors. (Measured and not kept, profiles/conv_fragment_ring.txt: a ring one set deeper, the staging loads
    // under the first four steps only, and a step's memory instructions all in front of its MFMAs -- 5 % slower than the
    // loop this one replaced.)
    constexpr int STEPS = TAPS * NGD;
    constexpr int D = 2;                                  // ring depth: the 24 registers the loop had (1x1: one chunk ahead)
    constexpr int NLD = BREG * 4;                         // staging dwords per thread and chunk
    constexpr int LPS = (NLD + STEPS - 1) / STEPS;        // ... issued under a step
    static_assert(D <= STEPS, "the fragment of step s + D is the current chunk's or the next one's");
    dm_f32x4 aq[D + 1][WM];      // the ring, oldest first: aq[0] is the step the MFMAs run, aq[D] the set being loaded
    auto stage_cursor = [&]() {      // the staging cursor moves to the chunk at (cs, cc0)
      if (b_src != cs) {
        const size_t bs = (size_t)a.src_bs[cs];
#pragma unroll
        for (int k = 0; k < NPOS; ++k) b_off[k] = (size_t)max(st_n[k], 0) * bs + st_pix[k];
        b_src = cs;
      }
      st_base = a.src[cs] + (size_t)cc0 * HW;
      st_ckv = min(CK, curC - cc0);
    };
    auto stage = [&](int l) {      // staging dword l of the cursor's chunk
      const int i = l / 4, e = l % 4;
      rb[i][e] = st_base[(size_t)min(st_channel(i, e), st_ckv - 1) * HW + b_off[KS == 3 ? i / NQ : 0]];
    };
    auto load_b = [&](int st, dm_f32x4* bv) {
      const int tap = st / NGD, g = st - tap * NGD;
      const int tapoff = (KS == 3) ? ((tap / 3) * Wp + (tap % 3)) : 0;
#pragma unroll
      for (int j = 0; j < WN; ++j) bv[j] = ldsB[(2 * g) * plane + lane_base[j] + tapoff];
    };
    if (chunk_valid()) {
      stage_cursor();
#pragma unroll
      for (int l = 0; l < NLD; ++l) stage(l);
#pragma unroll
      for (int d = 0; d < D; ++d) load_a(ckq, (st_ckv + 7) / 8, d, aq[d]);
    }
    while (chunk_valid()) {
      const int ngroups = (st_ckv + 7) / 8;   // quad pairs holding live channels
      const int ckq_cur = ckq;
      commit();
      __syncthreads();
      chunk_advance();
      --k_left;
      const bool more = chunk_valid();
      if (more) stage_cursor();
      const int ckq_nxt = more ? ckq : ckq_cur, ng_nxt = (st_ckv + 7) / 8;
      dm_f32x4 bv[2][WN];
      load_b(0, bv[0]);
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        const int cur = st & 1;
        const bool live = (NGD == 1) || ((st % NGD) < ngroups);
        if (st + 1 < STEPS) load_b(st + 1, bv[cur ^ 1]);
        if (st + D < STEPS) load_a(ckq_cur, ngroups, st + D, aq[D]);
        else load_a(ckq_nxt, ng_nxt, st + D - STEPS, aq[D]);
#pragma unroll
        for (int l = st * LPS; l < (st + 1) * LPS && l < NLD; ++l) stage(l);
        if (live) {
          // (s_setprio 1 around this cluster: +4 % in tools/micro/mfma_mix.hip, -3.5 % on the headline -- with three workgroups
          // per CU the prioritised waves starve the ones staging the next chunk)
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
              for (int j = 0; j < WN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[0][i][e], bv[cur][j][e], acc[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
          for (int i = 0; i < WM; ++i) aq[d][i] = aq[d + 1][i];
        // The scheduler, left alone, sinks the staging loads to the chunk's end and the fragment loads to one step ahead.  So
        // each step is a scheduling region of its own, and in it the memory instructions (NV loads, ND ds_reads) go one by one
        // between equal groups of the step's MFMAs.  (The builtin takes literal counts: hence the switch.)
        {
          const int NV = WM + max(0, min(LPS, NLD - st * LPS)), ND = st + 1 < STEPS ? WN : 0;
#pragma unroll
          for (int k = 0; k < NV + ND; ++k) {
            switch ((4 * WM * WN) / (NV + ND)) {
              case 0: case 1: __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); break;
              case 2: __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); break;
              case 3: __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); break;
              case 4: __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); break;
              default: __builtin_amdgcn_sched_group_barrier(0x008, 5, 0); break;
            }
            if (k < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read
            else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);             // DS read
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 4 * WM * WN, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }
  } else {
    if (chunk_valid()) prefetch();
    while (chunk_valid()) {
      const int ckv_cur = min(CK, curC - cc0);
      const int ngroups = (ckv_cur + 7) / 8;   // quad pairs holding live channels
      commit();
      __syncthreads();
      chunk_advance();
      --k_left;
      dm_f32x4 av[2][WM + (TAIL ? 1 : 0)], bv[2][WN];      // the exact builds' operand fragments
      if (chunk_valid()) prefetch();

      // ---- MFMA over the committed chunk ---------------------------------------
      // Operand fragments are double-buffered in registers: the ds_reads of step s+1 are
      // issued before the 4 x WM x WN MFMAs of step s, so LDS latency never stalls the
      // matrix pipe (the compiler alone re-uses one register set and issues them late).
      if (PREC) {
        // one step per tap: the chunk's 16 channels are ONE k of v_mfma_f32_32x32x16_bf16 (lane half hi = channels 8 hi ..)
        auto load_frag = [&](int tap, dm_f32x4 (*av)[3], dm_f32x4 (*bv)[3]) {
          const int tapoff = (KS == 3) ? ((tap / 3) * Wp + (tap % 3)) : 0;
#pragma unroll
          for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int p_ = 0; p_ < 3; ++p_) av[i][p_] = ldsA[(tap * NWC + 3 * hi + p_) * TMA + (wave_m * WM + i) * 32 + l31];
#pragma unroll
          for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int p_ = 0; p_ < 3; ++p_) bv[j][p_] = ldsB[p_ * plane + lane_base[j] + tapoff];
        };
        auto mfma = [&](const dm_f32x4& x, const dm_f32x4& y, dm_f32x16& c) {
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dm_bf16x8, x), __builtin_bit_cast(dm_bf16x8, y), c, 0, 0, 0);
        };
        dm_f32x4 av[2][WM][3], bv[2][WN][3];
        load_frag(0, av[0], bv[0]);
#pragma unroll
        for (int st = 0; st < TAPS; ++st) {
          const int cur = st & 1;
          if (st + 1 < TAPS) load_frag(st + 1, av[cur ^ 1], bv[cur ^ 1]);
#pragma unroll
          for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
              // (A part, B part), smallest terms first: the same order in every launch, hence the same bits every run.  The
              // five correction terms go to an accumulator of their own (~2^-8 of the main one: its roundings are that much
              // smaller), added to hi*hi's once, before the epilogue.
              mfma(av[cur][i][2], bv[cur][j][0], accx[i][j]);
              mfma(av[cur][i][1], bv[cur][j][1], accx[i][j]);
              mfma(av[cur][i][0], bv[cur][j][2], accx[i][j]);
              mfma(av[cur][i][1], bv[cur][j][0], accx[i][j]);
              mfma(av[cur][i][0], bv[cur][j][1], accx[i][j]);
              mfma(av[cur][i][0], bv[cur][j][0], acc[i][j]);
            }
        }
      } else {
        constexpr int NG = NQ / 2;
        constexpr int STEPS = TAPS * NG;
        auto load_frag = [&](int st, dm_f32x4* av, dm_f32x4* bv) {
          const int tap = st / NG, g = st - tap * NG;
          const int tapoff = (KS == 3) ? ((tap / 3) * Wp + (tap % 3)) : 0;
#pragma unroll
          for (int i = 0; i < WM; ++i)
            av[i] = ldsA[(tap * NQ + 2 * g + hi) * TMA + (wave_m * WM + i) * 32 + l31];
          if (TAIL) av[WM] = ldsA[(tap * NQ + 2 * g + hi) * TMA + TM + (lane & 3)];
#pragma unroll
          for (int j = 0; j < WN; ++j) bv[j] = ldsB[(2 * g) * plane + lane_base[j] + tapoff];
        };
        load_frag(0, av[0], bv[0]);
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {
          const int cur = st & 1;
          // quad pairs beyond the chunk's live channels hold zeros (1x1, ragged sources): skip them
          const bool live = (NG == 1) || ((st % NG) < ngroups);
          if (st + 1 < STEPS) load_frag(st + 1, av[cur ^ 1], bv[cur ^ 1]);
          if (live) {
            // (s_setprio 1 around this cluster: +4 % in tools/micro/mfma_mix.hip, -3.5 % on the headline -- with three workgroups
            // per CU the prioritised waves starve the ones staging the next chunk)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
                  acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i][e], bv[cur][j][e], acc[i][j], 0, 0, 0);
            if (TAIL) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < WN; ++j)
                  acct[j] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[cur][WM][e], bv[cur][j][e], acct[j], 0, 0, 0);
            }
          }
        }
      }
      __syncthreads();
    }

  }

  if (PREC) {
#pragma unroll
    for (int i = 0; i < WMX; ++i)
#pragma unroll
      for (int j = 0; j < WNX; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] += accx[i][j][r];
  }

  // ---- epilogue: bias + ReLU, 32 consecutive pixels per register ------------
  // Address arithmetic is hoisted: one 64-bit base per pixel column, one per-lane channel offset, the
  // rest is uniform (SALU); the store modes are uniform too and pick one of three straight-line
  // variants.  (Written naively -- the full index expression per store, mode tests inside -- the
  // epilogue was 3700 VALU instructions per wave, as many as the 32 chunks of the main loop together,
  // and VALU work is not free next to MFMAs: tools/micro/mfma_mix.hip.)
  if (a.shuffle == 0) {
    float* pj[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j)
      pj[j] = e_out + ((size_t)col_n[j] * e_oct + e_oco) * HW + col_p[j];
    const int co_lane = m0 + wave_m * WM * 32 + 4 * hi;
    const size_t off_lane = (size_t)co_lane * HW;
    const bool relu = e_relu & 1;
    // POST == 2: the addend is a smaller map of its own, gathered through the row and column tables.  One base per pixel
    // column (image, iy[y], ix[x]: the two lookups happen here, once, in front of the bias loads) and one per-lane channel
    // offset in the addend's own plane stride; the store loop adds a uniform k * up_plane, as it adds k * HW for out.
    const float* aj[WN];
    const int up_plane = POST == 2 ? a.up_plane : 0;
    const size_t aoff_lane = (size_t)co_lane * up_plane;
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      aj[j] = nullptr;
      if (POST == 2) {
        const int y = col_p[j] / W;          // (col_p is that of a pixel inside the map in every lane: q is clamped above)
        const int x = col_p[j] - y * W;
        aj[j] = a.addend + (size_t)col_n[j] * a.Cout * up_plane + (a.up_iy[y] * a.up_Ws + a.up_ix[x]);
      }
    }
    // all bias values first: a load inside the store loop puts an s_waitcnt vmcnt(0) -- which also
    // waits for the stores issued so far -- in front of every output row
    float bias_r[WM][16];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) bias_r[i][r] = 0.f;
    if (e_bias) {
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) bias_r[i][r] = e_bias[min(co_lane + i * 32 + (r & 3) + 8 * (r >> 2), a.Cout - 1)];
      // land them all here: otherwise the compiler waits for each value at its use, with counts that
      // include the stores issued meanwhile
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bias_r[i][r]));
    }
    const ptrdiff_t mask_off = e_mask ? e_mask - e_out : 0;
    const ptrdiff_t add_off = POST == 1 ? a.addend - e_out : 0;
    // full: the workgroup's tile lies inside the output (every cout row and every pixel column exists) -- uniform, and then
    // no store is predicated: the row and column tests cost an exec-mask sequence each, 600 scalar instructions per wave in
    // front of the 64 stores of a K = 64 GEMM (SQ counters: 4.8 SALU per MFMA on 64 -> 576 @56^2)
    // (1x1 builds only: in the 3x3 kernel the second copy of the epilogue cost 0.5 % of the headline, its K = 2304 loop hides the tests)
    const bool full = KS == 1 && m0 + TM <= a.Cout && q0 + TN <= a.Q;
    auto store_all = [&](auto acc_mode, auto nt_mode, auto mask_mode, auto full_mode) {
#pragma unroll
      for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = i * 32 + (r & 3) + 8 * (r >> 2);       // compile-time part of the channel
          if (decltype(full_mode)::value || co_lane + k < a.Cout) {
            const float b = bias_r[i][r];
            const size_t o = off_lane + (size_t)k * HW;
            const size_t ao = aoff_lane + (size_t)k * up_plane;
#pragma unroll
            for (int j = 0; j < WN; ++j) {
              if (decltype(full_mode)::value || col_ok[j]) {
                float* op = pj[j] + o;
                float v = acc[i][j][r] + b;
                if (decltype(acc_mode)::value) v += *op;          // accumulate into the destination (gradient sums)
                if (relu) v = dm_relu(v);
                if (POST == 2) v = aj[j][ao] + v;                 // (a map of its own: it never is out)
                else if (POST) v = op[add_off] + v;               // (read before this thread's own store: out may be the addend)
                if (decltype(mask_mode)::value) v = dm_relu_mask(op[mask_off], v);   // the producer's ReLU, looking backward
                if (decltype(nt_mode)::value) __builtin_nontemporal_store(v, op);   // output larger than the Infinity Cache: stream it
                else *op = v;
              }
            }
          }
        }
      }
    };
    using T = std::true_type;
    using F = std::false_type;
    if (KS == 1 && full) {
      if (e_mask) {
        if (e_relu & 2) store_all(T{}, F{}, T{}, T{});
        else store_all(F{}, F{}, T{}, T{});
      } else if (e_relu & 2) store_all(T{}, F{}, F{}, T{});
      else if (e_relu & 4) store_all(F{}, T{}, F{}, T{});
      else store_all(F{}, F{}, F{}, T{});
    } else if (e_mask) {
      if (e_relu & 2) store_all(T{}, F{}, T{}, F{});
      else store_all(F{}, F{}, T{}, F{});
    } else if (e_relu & 2) store_all(T{}, F{}, F{}, F{});
    else if (e_relu & 4) store_all(F{}, T{}, F{}, F{});
    else store_all(F{}, F{}, F{}, F{});
  } else {
    // deconv 2x2/s2: packed cout = phase * shuffle + oc, stored at (2y+dy, 2x+dx)
    int sy[WN], sx[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      sy[j] = col_p[j] / W;
      sx[j] = col_p[j] - sy[j] * W;
    }
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = m0 + (wave_m * WM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (co < a.Cout) {
          const int phase = co / a.shuffle;
          const int oc = co - phase * a.shuffle;
          const int dy = phase >> 1, dx = phase & 1;
          const float b = e_bias ? e_bias[oc] : 0.f;
#pragma unroll
          for (int j = 0; j < WN; ++j) {
            if (col_ok[j]) {
              float v = acc[i][j][r] + b;
              if (e_relu & 1) v = dm_relu(v);
              e_out[(((size_t)col_n[j] * a.shuffle + oc) * (2 * H) + 2 * sy[j] + dy) * (2 * W) + 2 * sx[j] + dx] = v;
            }
          }
        }
      }
    }
  }
  if (TAIL) {
    // the two lane halves hold the two K halves of the same pixels
#pragma unroll
    for (int j = 0; j < WN; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = acct[j][i] + __shfl_xor(acct[j][i], 32, 64);
        const int co = m0 + TM + i;
        if (hi == 0 && co < a.Cout && col_ok[j]) {
          if (e_bias) v += e_bias[co];
          float* op = e_out + ((size_t)col_n[j] * e_oct + e_oco + co) * HW + col_p[j];
          if (e_relu & 2) v += *op;
          if (e_relu & 1) v = dm_relu(v);
          if (e_mask) v = dm_relu_mask(e_mask[op - e_out], v);
          *op = v;
        }
      }
    }
  }
}

// (PREC 3x3: 55 KB of A image + the plane -- two workgroups per CU)
template <int KS, int WGM, int WGN, int WM, int WN, int CK, int MAXPOS, int TAIL = 0, int PREC = 0, int POST = 0>
__global__ __launch_bounds__(WGM* WGN * 64, PREC ? (KS == 1 ? 3 : 2) : (KS == 3 && WGM == 2 && WGN == 2 && WM == 2 && WN == 2 && MAXPOS == 1) || (KS == 1 && CK == 16) ? 3 : 1) void conv_igemm_kernel(ConvArgs a) {
  conv_igemm_body<KS, WGM, WGN, WM, WN, CK, MAXPOS, TAIL, PREC, POST>(a, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y);
}

// Up to three INDEPENDENT convolutions in one launch (round 6: the three FPN-wide semantic_transform_in 1x1 convolutions of
// the SFM stages, dynamask_head.py:104 -- P4 256->256, P3 256->128, P2 256->64: 66 / 132 / 525 workgroups that each walk
// a K = 256 loop, one launch after the other in front of everything else): workgroups [end[i-1], end[i]) run problem i
// with the body above, i.e. the same code on the same operands as a launch of its own.
struct ConvGroup {
  ConvArgs a[3];
  int end[3];
};
// (The cascade's stage-grouped 3x3 / 1x1 / deconv launches, dm_conv2d_group_fwd / dm_deconv2x2_group_fwd, run the same
// kernel: blockIdx.y is the K split of a grouped split-K launch, as in conv_igemm_kernel.)
template <int KS, int WGM, int WGN, int WM, int WN, int CK, int MAXPOS, int PREC = 0>
// (The 128 x 128 builds are held to two waves per SIMD here: at three they spill, 5 dwords for the 3x3 and 3 for the 1x1.)
__global__ __launch_bounds__(WGM* WGN * 64, (KS == 1 && CK == 16 && WM == 1) ? 3 : (WGM == 2 && WGN == 2 && WM == 2 && WN == 2) ? 2 : 1) void conv_igemm_group_kernel(ConvGroup g) {
  const int b = (int)blockIdx.x, by = (int)blockIdx.y;
  if (b < g.end[0]) conv_igemm_body<KS, WGM, WGN, WM, WN, CK, MAXPOS, 0, PREC>(g.a[0], b, g.end[0], by);
  else if (b < g.end[1]) conv_igemm_body<KS, WGM, WGN, WM, WN, CK, MAXPOS, 0, PREC>(g.a[1], b - g.end[0], g.end[1] - g.end[0], by);
  else conv_igemm_body<KS, WGM, WGN, WM, WN, CK, MAXPOS, 0, PREC>(g.a[2], b - g.end[1], g.end[2] - g.end[1], by);
}

// Packed weight layout [tap][KQ][CoutP][4]: KQ quads = sum over sources of
// roundup(Cs, 8)/4, channels of a source padded with zero rows to a multiple of 8.
struct PackArgs {
  const float* w;
  float* wq;
  int Cout, Cin, kk, flip;   // dims of the OIHW tensor
  int rows, cols, colsP;     // rows = reduction channels, cols = produced channels
  int nsrc;
  int src_c[DM_MAX_SOURCES];
  int KQ;
  int deconv;                // w is [Cin][Cout][2][2]; packed col = phase*Cout + co
};

__device__ __forceinline__ void pack_weight_body(const PackArgs& p, int ld, int c0) {
  // ld / c0: row length and first column of the [Cout][ld][k][k] tensor the packed [Cout][Cin] window sits in
  // (ld = Cin, c0 = 0: the whole tensor; a window = the input-channel slice of one concat source)
  const long long total = (long long)p.kk * p.KQ * p.colsP * 4;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(idx & 3);
    const int col = (int)((idx >> 2) % p.colsP);
    const int kq = (int)((idx >> 2) / p.colsP % p.KQ);
    const int tap = (int)((idx >> 2) / ((long long)p.colsP * p.KQ));
    // padded channel index -> (source, local channel) -> dense reduction row
    int pc = kq * 4 + e, row = -1, base = 0;
    for (int s = 0; s < p.nsrc; ++s) {
      const int padded = (p.src_c[s] + 7) / 8 * 8;
      if (pc < padded) {
        if (pc < p.src_c[s]) row = base + pc;
        break;
      }
      pc -= padded;
      base += p.src_c[s];
    }
    float v = 0.f;
    if (row >= 0 && col < p.cols) {
      if (p.deconv) {
        const int phase = col / p.Cout, co = col - phase * p.Cout;
        v = p.w[((size_t)row * p.Cout + co) * 4 + phase];
      } else if (!p.flip) {
        v = p.w[((size_t)col * ld + c0 + row) * p.kk + tap];               // col = co, row = ci
      } else {
        v = p.w[((size_t)row * ld + c0 + col) * p.kk + (p.kk - 1 - tap)];    // row = co, col = ci
      }
    }
    p.wq[idx] = v;
  }
}

__global__ void pack_weight_kernel(PackArgs p) { pack_weight_body(p, p.Cin, 0); }

// bf16x3 layout (PREC builds): [tap][KQ][colsP][16 bytes], sources padded to 16 channels, KQ = sum of roundup(Cs, 16) / 16
// * 6 words; word 6 b + 3 h + part of a source's 16-channel block b holds channels 16 b + 8 h .. + 7 of one produced
// channel as bf16 (part 0 = hi, 1 = mid, 2 = lo: dm_split3).  One thread per (tap, 8-channel half, col).
__global__ void pack_weight_bf16x3_kernel(PackArgs p) {
  const int HB = p.KQ / 3;                      // 8-channel halves
  const long long total = (long long)p.kk * HB * p.colsP;
  dm_f32x4* out = reinterpret_cast<dm_f32x4*>(p.wq);
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(idx % p.colsP);
    const int hb = (int)(idx / p.colsP % HB);
    const int tap = (int)(idx / ((long long)p.colsP * HB));
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int pc = hb * 8 + e, row = -1, base = 0;
      for (int s = 0; s < p.nsrc; ++s) {
        const int padded = (p.src_c[s] + 15) / 16 * 16;
        if (pc < padded) {
          if (pc < p.src_c[s]) row = base + pc;
          break;
        }
        pc -= padded;
        base += p.src_c[s];
      }
      float x = 0.f;
      if (row >= 0 && col < p.cols) {
        if (p.deconv) {
          const int phase = col / p.Cout, co = col - phase * p.Cout;
          x = p.w[((size_t)row * p.Cout + co) * 4 + phase];
        } else if (!p.flip) {
          x = p.w[((size_t)col * p.Cin + row) * p.kk + tap];
        } else {
          x = p.w[((size_t)row * p.Cin + col) * p.kk + (p.kk - 1 - tap)];
        }
      }
      v[e] = x;
    }
    dm_f32x4 wd[3];
    dm_split8x3(dm_f32x4{v[0], v[1], v[2], v[3]}, dm_f32x4{v[4], v[5], v[6], v[7]}, wd);
    const size_t w0 = ((size_t)tap * p.KQ + 3 * hb) * p.colsP + col;
#pragma unroll
    for (int p_ = 0; p_ < 3; ++p_) out[w0 + (size_t)p_ * p.colsP] = wd[p_];
  }
}

// Every pack of a training step in ONE launch (blockIdx.y = job): ~45 weight tensors change with every optimizer
// step, and a launch per tensor cost the host 1.3 ms of the 3.7 ms it needs to issue a forward pass.
__global__ void pack_weight_batch_kernel(const dm_pack_job* __restrict__ jobs) {
  const dm_pack_job j = jobs[blockIdx.y];
  PackArgs p;
  p.w = j.w; p.wq = j.w_packed; p.Cout = j.Cout; p.Cin = j.Cin; p.kk = j.ksize * j.ksize; p.flip = (j.transpose_flip & 1) ? 1 : 0;
  p.rows = p.flip ? j.Cout : j.Cin;
  p.cols = p.flip ? j.Cin : j.Cout;
  p.colsP = (p.cols + 31) / 32 * 32;
  p.nsrc = j.num_srcs;
  p.KQ = 0;
  for (int s = 0; s < DM_MAX_SOURCES; ++s) {
    p.src_c[s] = s < j.num_srcs ? j.src_channels[s] : 0;
    if (s < j.num_srcs) p.KQ += (j.src_channels[s] + 7) / 8 * 2;
  }
  p.deconv = 0;
  pack_weight_body(p, j.ld, j.c0);
}

int packed_quads(int nsrc, const int* src_c) {
  int kq = 0;
  for (int s = 0; s < nsrc; ++s) kq += (src_c[s] + 7) / 8 * 2;
  return kq;
}

int packed_words_bf16x3(int nsrc, const int* src_c) {
  int kq = 0;
  for (int s = 0; s < nsrc; ++s) kq += (src_c[s] + 15) / 16 * 6;
  return kq;
}

// out = epilogue(sum over the splits, in index order): the conv kernel's own epilogue arithmetic (bias, accumulate, ReLU,
// mask -- in that order) on the bare sums of a split-K launch.  ws: [splits][NB][Cout][HW]; out / mask: [NB][out_ch_total][HW].
// (round 5: four outputs per thread and 32-bit index arithmetic where HW % 4 == 0 and everything is 16-byte aligned --
// one thread per output with two 64-bit divisions took 27 us for the 2.5 M outputs of a 50-RoI convolution, 1.5 TB/s.)
template <bool V4>
__device__ __forceinline__ void splitk_reduce_body(const float* __restrict__ ws, int splits, long long stride, int NB, int Cout,
                                                   int HW, const float* __restrict__ bias, int flags, float* __restrict__ out,
                                                   int out_ch_total, int out_ch_offset, const float* __restrict__ mask) {
  if (V4) {
    // total = NB * Cout * HW < 2^31 (launcher); a quad never straddles a channel plane (HW % 4 == 0)
    const unsigned total4 = (unsigned)(((long long)NB * Cout * HW) >> 2), hw4 = (unsigned)HW >> 2;
    const float4* ws4 = reinterpret_cast<const float4*>(ws);
    const size_t stride4 = (size_t)(stride >> 2);
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total4; e += gridDim.x * blockDim.x) {
      const unsigned nc = e / hw4, p4 = e - nc * hw4;
      const unsigned n = nc / (unsigned)Cout, co = nc - n * (unsigned)Cout;
      float4 v = ws4[e];
      for (int s = 1; s < splits; ++s) {
        const float4 w = ws4[(size_t)s * stride4 + e];
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
      }
      if (bias) {
        const float bv = bias[co];
        v.x += bv; v.y += bv; v.z += bv; v.w += bv;
      }
      const size_t o4 = ((size_t)n * out_ch_total + out_ch_offset + co) * hw4 + p4;
      float4* op = reinterpret_cast<float4*>(out) + o4;
      if (flags & 2) {
        const float4 w = *op;
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
      }
      if (flags & 1) { v.x = dm_relu(v.x); v.y = dm_relu(v.y); v.z = dm_relu(v.z); v.w = dm_relu(v.w); }
      if (mask) {
        const float4 m = reinterpret_cast<const float4*>(mask)[o4];
        v.x = dm_relu_mask(m.x, v.x); v.y = dm_relu_mask(m.y, v.y); v.z = dm_relu_mask(m.z, v.z); v.w = dm_relu_mask(m.w, v.w);
      }
      *op = v;
    }
    return;
  }
  const long long total = (long long)NB * Cout * HW;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long nc = e / HW;
    const int p = (int)(e - nc * HW);
    const int n = (int)(nc / Cout), co = (int)(nc - (long long)n * Cout);
    float v = ws[e];
    for (int s = 1; s < splits; ++s) v += ws[(size_t)s * stride + e];
    if (bias) v += bias[co];
    const size_t o = ((size_t)n * out_ch_total + out_ch_offset + co) * HW + p;
    if (flags & 2) v += out[o];
    if (flags & 1) v = dm_relu(v);
    if (mask) v = dm_relu_mask(mask[o], v);
    out[o] = v;
  }
}

template <bool V4>
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const float* __restrict__ ws, int splits, long long stride, int NB,
                                                                int Cout, int HW, const float* __restrict__ bias, int flags,
                                                                float* __restrict__ out, int out_ch_total, int out_ch_offset,
                                                                const float* __restrict__ mask) {
  splitk_reduce_body<V4>(ws, splits, stride, NB, Cout, HW, bias, flags, out, out_ch_total, out_ch_offset, mask);
}

// The reduction of a grouped split-K launch: blockIdx.y = problem, whose splits lie at ws[p] (the same arithmetic as
// conv_splitk_reduce_kernel; bias and ReLU only, outputs [NB][Cout][HW] of their own).
struct ReduceGroup {
  const float* ws[3];
  const float* bias[3];
  float* out[3];
};
template <bool V4>
__global__ __launch_bounds__(256) void conv_splitk_reduce_group_kernel(ReduceGroup r, int splits, long long stride, int NB,
                                                                      int Cout, int HW, int flags) {
  const int p = (int)blockIdx.y;
  splitk_reduce_body<V4>(r.ws[p], splits, stride, NB, Cout, HW, r.bias[p], flags, r.out[p], Cout, 0, nullptr);
}

// The constants of one build of the kernel: a workgroup of NT threads computes TM (+ TAIL) couts x TN pixels and walks K in
// chunks of NWC 16-byte words per cout / plane position.  The launchers, and nothing else, read it.
template <int KS_, int WGM_, int WGN_, int WM_, int WN_, int CK_, int TAIL_, int PREC_>
struct ConvBuild {
  static constexpr int KS = KS_, WGM = WGM_, WGN = WGN_, WM = WM_, WN = WN_, CK = CK_, TAIL = TAIL_, PREC = PREC_;
  static constexpr int TM = WGM * WM * 32, TN = WGN * WN * 32, NT = WGM * WGN * 64, NWC = PREC ? 6 : CK / 4;
  static constexpr bool DIRECT = conv_direct_a<KS, WGM, WGN, WM, WN, CK, TAIL, PREC>();      // no A image: the B planes only
  static constexpr size_t lds_bytes(int plane) {
    return 16 * ((DIRECT ? 0 : (size_t)KS * KS * NWC * (TM + TAIL)) + (size_t)NWC * plane);
  }
  // (the fragment loads of a DIRECT build address the packed weights through a buffer descriptor with 32-bit byte offsets)
  static bool weights_addressable(const ConvArgs& a) { return !DIRECT || (long long)KS * KS * a.KQ * a.CoutP * 16 <= 0x7fffffffLL; }
};

// Positions of the plane a 3x3 workgroup stages for a tile of TN flat pixels: the rows the tile's pixels touch plus a halo
// row above and below each image segment of the tile, each row W + 2 wide
int conv_plane(int TN, int H, int W) {
  const int nsegmax = dm_ceil_div(TN - 1, H * W) + 1;
  return (dm_ceil_div(TN - 1, W) + 1 + 2 * nsegmax) * (W + 2);
}

// The geometry of problems a[0 .. n) under build B (MT, Wp, plane), then f(MAXPOS) for the build that stages a[0]'s plane
// with B's NT threads: 1, 2 or 4 positions per thread (1x1: no plane, 1).  bf16x3: one position per thread only (maps up
// to ~16 x 16); wider maps would need more than 80 KB of LDS.
template <class B, class F>
int conv_with_maxpos(ConvArgs* a, int n, F&& f) {
  for (int i = 0; i < n; ++i) {
    a[i].MT = B::TAIL ? 1 : dm_ceil_div(a[i].CoutP, B::TM);
    a[i].Wp = B::KS == 3 ? a[i].W + 2 : 0;
    a[i].plane = B::KS == 3 ? conv_plane(B::TN, a[i].H, a[i].W) : B::TN;
  }
  const int plane = a[0].plane;
  if (B::KS == 1 || plane <= B::NT) return f(std::integral_constant<int, 1>());
  if constexpr (B::KS == 3 && B::PREC == 0) {
    if (plane <= 2 * B::NT) return f(std::integral_constant<int, 2>());
    if (plane <= 4 * B::NT) return f(std::integral_constant<int, 4>());
  }
  return DM_ERR_UNSUPPORTED;
}
// (The exact 1x1 builds at 2 and 4 positions per thread: no launch reaches them -- a 1x1 tile has no plane -- but the ladder
// used to instantiate them, and they stay in the code object until a change that measures the library without them.)
#define DM_CONV_UNREACHED(...) \
  template __global__ void conv_igemm_kernel<1, __VA_ARGS__, 2>(ConvArgs); \
  template __global__ void conv_igemm_kernel<1, __VA_ARGS__, 4>(ConvArgs)
DM_CONV_UNREACHED(1, 4, 1, 1, 32);
DM_CONV_UNREACHED(2, 2, 1, 2, 16);
DM_CONV_UNREACHED(2, 2, 2, 2, 16);
DM_CONV_UNREACHED(4, 1, 1, 1, 32);
#undef DM_CONV_UNREACHED

// Launches that do not fill the chip take 128 x 32 tiles instead of 128 x 128 (3x3, Cout > 64): up to one 128 x 128 tile per
// CU costs a lone workgroup's 0.18 ms however few there are, up to two 0.31 ms; 128 x 32 tiles cost 0.04 + 0.046 ms per
// tile-per-CU (16 RoIs of 14 x 14: 0.175 -> 0.077 ms, 100 RoIs: 0.322 -> 0.275 ms).  wgs: the launch's 128 x 128 tiles.
bool conv_small_launch(int wgs, int cus) { return wgs * 10 <= cus * 7 || (wgs > cus && wgs * 20 <= cus * 29); }

// K chunks of CK channels a launch walks: every source is padded to whole chunks
int conv_chunks(int num_srcs, const int* src_c, int CK) {
  int chunks = 0;
  for (int s = 0; s < num_srcs; ++s) chunks += dm_ceil_div(src_c[s], CK);
  return chunks;
}

// How many K splits pay for a launch that leaves most of the chip idle (1: none).  A launch of one round walks its chunks
// one after the other at ~2.1 us (3x3) / ~1.5 us (1x1) per chunk whatever the RoI count (tools/small_n.py: conv14 64-71 us
// for 32 chunks, fuse14 50 us for 33); S splits save (1 - 1/S) of that and cost a second launch (~5 us) that reads S and
// writes one copy of the output at ~4 TB/s; at least 8 us of net gain.
// (Without this test the 1x1 convolutions of the 28 x 28 / 56 x 56 stages split too: 17.7 reduce launches of 15.7 us
// each per 100-detection call, more than the splits saved.)
int conv_split_choice(int chunks, bool k3, int Smax, long long out_floats) {
  const double chain_us = chunks * (k3 ? 2.1 : 1.5), out_mb = (double)out_floats * 4e-6;
  double best = 8.0;
  int S = 1;
  for (int c = 2; c <= Smax; ++c) {
    const double g = chain_us * (1.0 - 1.0 / c) - (5.0 + (c + 1) * out_mb * 0.25);
    if (g > best) { best = g; S = c; }
  }
  return S;
}

// The splits `wgs` workgroups have room for on `slots` resident workgroups (slots per CU differ by build and caller, on purpose)
int conv_split_max(long long wgs, long long slots, int cap = 8) { return (int)min((long long)cap, slots / max(wgs, 1LL)); }

// The K split of a launch: S, the cost model's choice among the splits there is room for -- slots, at least four chunks per
// split, one out_floats-sized slice of the ws_floats workspace per split -- run as kchunks = ceil(chunks / S) chunks per split
// in ksplit = ceil(chunks / kchunks) <= S workgroups per tile (the workspace is laid out for S).
struct ConvSplit { int S = 1, ksplit = 1, kchunks = 0; };
ConvSplit conv_split(int chunks, bool k3, long long wgs, long long slots, long long ws_floats, long long out_floats, int cap = 8) {
  long long Smax = min(conv_split_max(wgs, slots, cap), chunks / 4);
  if (out_floats > 0) Smax = min(Smax, ws_floats / out_floats);
  ConvSplit k;
  k.S = conv_split_choice(chunks, k3, (int)Smax, out_floats);
  if (k.S >= 2) {
    k.kchunks = dm_ceil_div(chunks, k.S);
    k.ksplit = dm_ceil_div(chunks, k.kchunks);
  }
  return k;
}

// The one place a convolution kernel is enqueued -- or, under a recorder (dm_conv2d_plan / dm_conv2d_group_plan), written
// down instead: problems a[0 .. count) of build B in ONE launch, problem i on workgroups [end[i - 1], end[i]) of grid x,
// grid y the K split they share.  One record per problem, DM_CONV_PLAN_INTS ints in the order the header documents.
template <class B, int MAXPOS, int POST, class Enqueue>
int conv_emit(const ConvArgs* a, const int* end, int count, Enqueue&& enqueue) {
  const int splits = a[0].ksplit;
  if (ConvPlan* plan = a[0].plan) {
    if (plan->count + count > plan->cap) return DM_ERR_INVALID_ARG;
    for (int i = 0; i < count; ++i) {
      const int rec[DM_CONV_PLAN_INTS] = {B::KS, B::WGM, B::WGN, B::WM, B::WN, B::CK, B::TAIL, B::PREC, POST, MAXPOS,
                                          splits, splits > 1 ? a[i].kchunks : 0, a[i].q_begin, a[i].Q,
                                          end[i] - (i ? end[i - 1] : 0), splits, (a[i].relu & 4) ? 1 : 0};
      for (int k = 0; k < DM_CONV_PLAN_INTS; ++k) plan->rec[plan->count][k] = rec[k];
      plan->count++;
    }
    return DM_OK;
  }
  enqueue(dim3((unsigned)end[count - 1], (unsigned)splits));
  return dm_check_launch();
}

// The reduce after a split launch of `count` problems whose bare sums lie at r.ws[p]: conv_splitk_reduce_group_kernel
// (grouped: bias and ReLU only, outputs of their own) or conv_splitk_reduce_kernel (one problem, with a's output slice and mask)
int launch_splitk_reduce(const ReduceGroup& r, int count, bool grouped, const ConvArgs& a, int flags, hipStream_t st) {
  const long long per = a.ws_stride;
  uintptr_t addr = (uintptr_t)a.mask;
  for (int p = 0; p < count; ++p) addr |= (uintptr_t)r.ws[p] | (uintptr_t)r.out[p];
  // four outputs per thread where a quad never straddles a channel plane and everything is 16-byte aligned
  const bool v4 = (a.HW & 3) == 0 && (per & 3) == 0 && per < 0x7fffffffLL && (addr & 15) == 0;
  const dim3 grid((unsigned)min((long long)4096, ((v4 ? per / 4 : per) + 255) / 256), grouped ? (unsigned)count : 1u);
  auto enqueue = [&](auto V4) {
    if (grouped)
      DM_LAUNCH(conv_splitk_reduce_group_kernel<decltype(V4)::value>, grid, dim3(256), 0, st, r, a.ksplit, per, a.NB, a.Cout, a.HW, flags);
    else
      DM_LAUNCH(conv_splitk_reduce_kernel<decltype(V4)::value>, grid, dim3(256), 0, st, r.ws[0], a.ksplit, per, a.NB, a.Cout, a.HW, r.bias[0],
                flags, r.out[0], a.out_ch_total, a.out_ch_offset, a.mask);
  };
  v4 ? enqueue(std::true_type()) : enqueue(std::false_type());
  return dm_check_launch();
}

// One lone launch of build B at MAXPOS positions per thread: the LDS of the build, the K split (a caller-provided workspace,
// one launch per call), the launch and its reduce
template <class B, int MAXPOS, int POST>
int launch_conv_mp(ConvArgs& a, hipStream_t st) {
  const int wgs = a.MT * dm_ceil_div(a.Q - a.q_begin, B::TN);
  const size_t lds_bytes = B::lds_bytes(a.plane);
  if (!B::weights_addressable(a)) return DM_ERR_UNSUPPORTED;
  if (lds_bytes > 64 * 1024) {
    // (the bf16x3 3x3 build: 54 KB of A image + 21 KB of plane at 14 x 14; two workgroups per CU.  The exact 128-cout 3x3
    // builds whose plane holds more than 896 positions -- 36 KB of A image + 32 bytes per position: maps 148 .. 168 wide,
    // and narrower single-row ones, 1 x 100: 9 rows of 102 -- while the 64- and 32-cout builds stage every plane up to the
    // 1024-position limit in 64 KB: whether a map can be staged must not depend on Cout.  launch_group_mp raises no limit:
    // a grouped launch of such a plane is refused.)
    if (lds_bytes > 80 * 1024) return DM_ERR_UNSUPPORTED;
    if (!a.plan) {
      static bool raised[DM_MAX_DEVICES] = {false};
      const int rc = dm_ensure_lds_limit(
          reinterpret_cast<const void*>(&conv_igemm_kernel<B::KS, B::WGM, B::WGN, B::WM, B::WN, B::CK, MAXPOS, B::TAIL, B::PREC, POST>),
          80 * 1024, raised);
      if (rc != DM_OK) return rc;
    }
  }
  // ---- split-K for launches that leave most of the chip idle, on three slots per CU or as far as conv2d_launch decided
  a.ksplit = 1;
  if (a.ws && a.shuffle == 0 && a.q_begin == 0 && !POST) {
    const long long per = (long long)a.NB * a.Cout * a.HW;
    const ConvSplit k = conv_split(conv_chunks(a.num_srcs, a.src_c, B::CK), B::KS == 3, wgs, 3LL * dm_num_cus(), a.ws_floats, per,
                                   a.want_split > 0 ? a.want_split : 8);
    if (k.S >= 2) {
      a.kchunks = k.kchunks;
      a.ksplit = k.ksplit;
      a.ws_stride = per;
    }
  }
  const int rc = conv_emit<B, MAXPOS, POST>(&a, &wgs, 1, [&](dim3 grid) {
    DM_LAUNCH((conv_igemm_kernel<B::KS, B::WGM, B::WGN, B::WM, B::WN, B::CK, MAXPOS, B::TAIL, B::PREC, POST>), grid, dim3(B::NT),
              lds_bytes, st, a);
  });
  if (rc != DM_OK || a.plan || a.ksplit < 2) return rc;
  const ReduceGroup r = {{a.ws}, {a.bias}, {a.out}};
  return launch_splitk_reduce(r, 1, false, a, a.relu, st);
}

template <int KS, int WGM, int WGN, int WM, int WN, int CK, int TAIL = 0, int PREC = 0, int POST = 0>
int launch_conv(ConvArgs& a, hipStream_t st) {
  using B = ConvBuild<KS, WGM, WGN, WM, WN, CK, TAIL, PREC>;
  return conv_with_maxpos<B>(&a, 1, [&](auto mp) { return launch_conv_mp<B, decltype(mp)::value, POST>(a, st); });
}

// One grouped launch (dm_conv2d_group_fwd / dm_deconv2x2_group_fwd / dm_conv1x1_group_fwd) of the problems g.a[0 .. count),
// each in its own range of the grid, and -- k.S >= 2, problems of one shape, shuffle == 0 -- the K loop split over k.ksplit
// workgroups per tile exactly as launch_conv_mp splits a lone launch, with problem p's bare sums at ws + p * k.S * per,
// reduced by ONE conv_splitk_reduce_group_kernel.
template <class B, int MAXPOS>
int launch_group_mp(ConvGroup& g, int count, const ConvSplit& k, float* ws, hipStream_t st) {
  const ConvArgs& a0 = g.a[0];
  const size_t lds_bytes = B::lds_bytes(a0.plane);
  for (int i = 0; i < count; ++i)
    if (!B::weights_addressable(g.a[i])) return DM_ERR_UNSUPPORTED;
  if (lds_bytes > 64 * 1024) return DM_ERR_UNSUPPORTED;      // (where launch_conv_mp raises the limit: its comment)
  const long long per = (long long)a0.NB * a0.Cout * a0.HW;
  int total = 0;
  for (int i = 0; i < 3; ++i) {
    ConvArgs& a = g.a[i];
    a.ksplit = k.ksplit;
    if (k.S >= 2) {
      a.kchunks = k.kchunks;
      a.ws = ws + (size_t)min(i, count - 1) * k.S * per;
      a.ws_stride = per;
      a.ws_floats = (long long)k.S * per;
    }
    if (i < count) total += a.MT * dm_ceil_div(a.Q, B::TN);
    g.end[i] = total;
  }
  const int rc = conv_emit<B, MAXPOS, 0>(g.a, g.end, count, [&](dim3 grid) {
    DM_LAUNCH((conv_igemm_group_kernel<B::KS, B::WGM, B::WGN, B::WM, B::WN, B::CK, MAXPOS, B::PREC>), grid, dim3(B::NT), lds_bytes, st, g);
  });
  if (rc != DM_OK || a0.plan || a0.ksplit < 2) return rc;
  ReduceGroup r;
  for (int i = 0; i < 3; ++i) {
    const ConvArgs& a = g.a[min(i, count - 1)];
    r.ws[i] = a.ws; r.bias[i] = a.bias; r.out[i] = a.out;
  }
  return launch_splitk_reduce(r, count, true, a0, a0.relu & 1, st);
}

template <int KS, int WGM, int WGN, int WM, int WN, int CK, int PREC = 0>
int launch_group(ConvGroup& g, int count, const ConvSplit& k, float* ws, hipStream_t st) {
  using B = ConvBuild<KS, WGM, WGN, WM, WN, CK, 0, PREC>;
  return conv_with_maxpos<B>(g.a, 3, [&](auto mp) { return launch_group_mp<B, decltype(mp)::value>(g, count, k, ws, st); });
}

// The K split of a grouped 3x3 launch for a workspace of ws_floats: the decision conv2d_launch / launch_conv_mp make for ONE
// problem of this shape, taken on the grouped workgroup count -- a grouped launch fills more of the chip and splits less.
// The cost model is the lone launch's (per-problem output size, each problem's share of the workspace), so a lone
// dm_conv2d_fwd_ws given S problem-sized workspaces picks the same S (its Smax is then S, and S is the first maximum of
// the model below any larger Smax).  1x1 problems never split here.
ConvSplit group_split(int count, int NB, int H, int W, int Cin, int Cout, int ksize, long long ws_floats) {
  if (ksize != 3 || NB <= 0 || ws_floats <= 0) return ConvSplit();
  const long long per = (long long)NB * Cout * H * W;
  const long long Q = (long long)NB * H * W;
  const int cus = dm_num_cus();
  // (the grouped 128 x 128 build runs two workgroups per CU: conv_igemm_group_kernel's bounds; the 64 / 32 x 128 builds three)
  const long long slots = Cout > 64 ? 2LL * cus : 3LL * cus;
  const long long wgs = (long long)count * (Cout > 64 ? dm_ceil_div(dm_conv_packed_cout(Cout), 128) : 1) * dm_ceil_div(Q, 128);
  return conv_split(dm_ceil_div(Cin, 8), true, wgs, slots, ws_floats / count, per);
}

// Fills a: the arguments of one convolution as the kernel reads them, for every entry point -- the sources (src_bs null:
// dense), the map, the packed weights (bf16x3: that layout) and the `couts` packed columns, the flags as the kernel takes
// them, the output slice, the deconv's shuffle.  Everything else keeps ConvArgs' defaults.
int conv_fill(ConvArgs& a, const float* const* srcs, const int* src_c, const long long* src_bs, int num_srcs, int NB, int H, int W,
              const float* wq, bool bf16x3, const float* bias, int couts, int flags, float* out, int out_ch_total,
              int out_ch_offset, int shuffle) {
  a = ConvArgs();          // (zeroes: the sources past num_srcs are null and empty)
  a.off32 = 1;
  for (int s = 0; s < num_srcs; ++s) {
    if (!srcs[s] || src_c[s] <= 0) return DM_ERR_INVALID_ARG;
    a.src[s] = srcs[s];
    a.src_c[s] = src_c[s];
    a.src_bs[s] = src_bs ? src_bs[s] : (long long)src_c[s] * H * W;
    if (a.src_bs[s] < (long long)src_c[s] * H * W) return DM_ERR_INVALID_ARG;
    if ((long long)NB * a.src_bs[s] * 4 >= (1LL << 32)) a.off32 = 0;
  }
  a.num_srcs = num_srcs;
  a.KQ = bf16x3 ? packed_words_bf16x3(num_srcs, src_c) : packed_quads(num_srcs, src_c);
  a.NB = NB; a.H = H; a.W = W; a.HW = H * W; a.Q = NB * H * W;
  a.wq = wq; a.bias = bias; a.Cout = couts; a.CoutP = dm_conv_packed_cout(couts);
  a.relu = flags; a.out = out; a.out_ch_total = out_ch_total; a.out_ch_offset = out_ch_offset;
  a.shuffle = shuffle;
  return DM_OK;
}

// outputs that cannot stay in the 256 MB Infinity Cache next to their consumer's other traffic are
// written with nontemporal stores (measured: -10 % on the 1.85 GB column-gradient GEMM, neutral
// below): the launchers' own flag bit 2
int conv_store_policy(int NB, int Cout, int H, int W) { return (long long)NB * Cout * H * W * 4 > (192LL << 20) ? 4 : 0; }

int run_pack_bf16x3(PackArgs& p, hipStream_t st) {
  const long long total = (long long)p.kk * (p.KQ / 3) * p.colsP;
  const int blocks = (int)min((long long)dm_ceil_div(total, 256), 4096LL);
  DM_LAUNCH(pack_weight_bf16x3_kernel, dim3(blocks), dim3(256), 0, st, p);
  return dm_check_launch();
}

int run_pack(PackArgs& p, hipStream_t st) {
  const long long total = (long long)p.kk * p.KQ * p.colsP * 4;
  const int blocks = (int)min((long long)dm_ceil_div(total, 256), 4096LL);
  DM_LAUNCH(pack_weight_kernel, dim3(blocks), dim3(256), 0, st, p);
  return dm_check_launch();
}

}  // namespace

extern "C" int dm_conv_packed_cout(int Cout) { return (Cout + 31) / 32 * 32; }

extern "C" long long dm_conv_packed_floats(int Cout, int ksize, int num_srcs, const int* src_channels) {
  if (Cout <= 0 || ksize <= 0 || num_srcs < 1 || num_srcs > DM_MAX_SOURCES || !src_channels) return -1;
  return (long long)ksize * ksize * packed_quads(num_srcs, src_channels) * dm_conv_packed_cout(Cout) * 4;
}

extern "C" int dm_conv_pack_weight(const float* w_oihw, int Cout, int Cin, int ksize, int transpose_flip,
                                   int num_srcs, const int* src_channels, float* w_packed, dm_stream_t stream) {
  if (!w_oihw || !w_packed || Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return DM_ERR_INVALID_ARG;
  if (num_srcs < 1 || num_srcs > DM_MAX_SOURCES || !src_channels) return DM_ERR_INVALID_ARG;
  PackArgs p;
  p.w = w_oihw; p.wq = w_packed; p.Cout = Cout; p.Cin = Cin; p.kk = ksize * ksize; p.flip = transpose_flip ? 1 : 0;
  p.rows = transpose_flip ? Cout : Cin;
  p.cols = transpose_flip ? Cin : Cout;
  p.colsP = dm_conv_packed_cout(p.cols);
  p.nsrc = num_srcs;
  int sum = 0;
  for (int s = 0; s < DM_MAX_SOURCES; ++s) {
    p.src_c[s] = s < num_srcs ? src_channels[s] : 0;
    if (s < num_srcs && src_channels[s] <= 0) return DM_ERR_INVALID_ARG;
    sum += p.src_c[s];
  }
  if (sum != p.rows) return DM_ERR_INVALID_ARG;
  p.KQ = packed_quads(num_srcs, src_channels);
  p.deconv = 0;
  return run_pack(p, (hipStream_t)stream);
}

// (ABI 28) the bf16x3 layout of the same weights (the kernel's header): flag bit 4 of dm_conv2d_fwd / _ws /
// dm_conv1x1_group_fwd reads it
extern "C" long long dm_conv_packed_floats_bf16x3(int Cout, int ksize, int num_srcs, const int* src_channels) {
  if (Cout <= 0 || ksize <= 0 || num_srcs < 1 || num_srcs > DM_MAX_SOURCES || !src_channels) return -1;
  return (long long)ksize * ksize * packed_words_bf16x3(num_srcs, src_channels) * dm_conv_packed_cout(Cout) * 4;
}

extern "C" int dm_conv_pack_weight_bf16x3(const float* w_oihw, int Cout, int Cin, int ksize, int transpose_flip,
                                          int num_srcs, const int* src_channels, float* w_packed, dm_stream_t stream) {
  if (!w_oihw || !w_packed || Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return DM_ERR_INVALID_ARG;
  if (num_srcs < 1 || num_srcs > DM_MAX_SOURCES || !src_channels) return DM_ERR_INVALID_ARG;
  PackArgs p;
  p.w = w_oihw; p.wq = w_packed; p.Cout = Cout; p.Cin = Cin; p.kk = ksize * ksize; p.flip = transpose_flip ? 1 : 0;
  p.rows = transpose_flip ? Cout : Cin;
  p.cols = transpose_flip ? Cin : Cout;
  p.colsP = dm_conv_packed_cout(p.cols);
  p.nsrc = num_srcs;
  int sum = 0;
  for (int s = 0; s < DM_MAX_SOURCES; ++s) {
    p.src_c[s] = s < num_srcs ? src_channels[s] : 0;
    if (s < num_srcs && src_channels[s] <= 0) return DM_ERR_INVALID_ARG;
    sum += p.src_c[s];
  }
  if (sum != p.rows) return DM_ERR_INVALID_ARG;
  p.KQ = packed_words_bf16x3(num_srcs, src_channels);
  p.deconv = 0;
  return run_pack_bf16x3(p, (hipStream_t)stream);
}

extern "C" int dm_conv_pack_weight_batch(const dm_pack_job* jobs_device, int num_jobs, dm_stream_t stream) {
  if (num_jobs < 0 || (num_jobs > 0 && !jobs_device)) return DM_ERR_INVALID_ARG;
  if (num_jobs == 0) return DM_OK;
  if (num_jobs > 65535) return DM_ERR_INVALID_ARG;
  DM_LAUNCH(pack_weight_batch_kernel, dim3(64, (unsigned)num_jobs), dim3(256), 0, (hipStream_t)stream, jobs_device);
  return dm_check_launch();
}

// (K31) the gather of dm_conv2d_up_add_fwd's addend: [NB, Cout, Hs, Ws] read at (iy[y], ix[x])
struct UpAdd {
  int Hs, Ws;
  const int* iy;
  const int* ix;
};

// One launch of `a` with the epilogue the call asks for: plain, the post-activation addend (K26) or the gathered one (K31)
template <int KS, int WGM, int WGN, int WM, int WN, int CK>
static int launch_conv_post(ConvArgs& a, hipStream_t st) {
  if (!a.addend) return launch_conv<KS, WGM, WGN, WM, WN, CK>(a, st);
  if (a.up_iy) return launch_conv<KS, WGM, WGN, WM, WN, CK, 0, 0, 2>(a, st);
  return launch_conv<KS, WGM, WGN, WM, WN, CK, 0, 0, 1>(a, st);
}

static int conv2d_launch(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                         int num_srcs, int NB, int H, int W,
                         const float* w_packed, const float* bias, int Cout, int ksize, int relu, float* out,
                         int out_ch_total, int out_ch_offset, const float* mask, dm_stream_t stream, float* ws = nullptr,
                         long long ws_floats = 0, const float* addend = nullptr, ConvPlan* plan = nullptr,
                         const UpAdd* up = nullptr) {
  if (mask && (relu & 16)) return DM_ERR_UNSUPPORTED;      // (no bf16x3 build of the data-gradient launches)
  if (!srcs || !src_channels || num_srcs < 1 || num_srcs > DM_MAX_SOURCES || !w_packed || !out) return DM_ERR_INVALID_ARG;
  if (NB < 0 || H <= 0 || W <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3)) return DM_ERR_INVALID_ARG;
  if (out_ch_offset < 0 || out_ch_offset + Cout > out_ch_total) return DM_ERR_INVALID_ARG;
  if ((long long)NB * H * W > 0x7fffffffLL) return DM_ERR_INVALID_ARG;
  if (NB == 0) return DM_OK;
  if (relu & ~(1 | 2 | 8 | 16)) return DM_ERR_INVALID_ARG;      // (bit 2 is the launcher's own store-policy bit; bit 5 selected a bf16-split layout of ABI 18-21: removed)
  const bool bf16x3 = (relu & 16) != 0;          // (ABI 28) w_packed is the bf16x3 layout (dm_conv_pack_weight_bf16x3)
  ConvArgs a;
  const int rc = conv_fill(a, srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, w_packed, bf16x3, bias, Cout, relu & 3, out,
                           out_ch_total, out_ch_offset, 0);
  if (rc != DM_OK) return rc;
  a.plan = plan;
  a.mask = mask;
  a.ws = (ws && ws_floats > 0) ? ws : nullptr;
  a.ws_floats = ws_floats;
  // (accumulating launches read the destination and keep the default store policy)
  if (!(relu & 2)) a.relu |= conv_store_policy(NB, Cout, H, W);
  hipStream_t st = (hipStream_t)stream;
  if (addend) {
    // (K26) the POST builds: exact fp32 1x1, flags ReLU only, no split, default store policy
    if (ksize != 1 || bf16x3) return DM_ERR_UNSUPPORTED;
    if ((relu & ~1) || mask) return DM_ERR_INVALID_ARG;
    a.addend = addend;
    a.relu = relu & 1;
    a.ws = nullptr;
    if (up) {
      a.up_iy = up->iy;
      a.up_ix = up->ix;
      a.up_Ws = up->Ws;
      a.up_plane = up->Hs * up->Ws;
    }
  }
  if (bf16x3) {
    // one build per kernel size: 64 couts x 128 pixels, four waves of 32 x 64 (see the kernel's header); a workspace
    // lets it split K as the exact launches do (conv_split's cost model, 16-channel chunks)
    if (ksize == 3) return launch_conv<3, 2, 2, 1, 2, 16, 0, 1>(a, st);
    return launch_conv<1, 2, 2, 1, 2, 16, 0, 1>(a, st);
  }
  if (ksize == 3) {
    if (Cout > 64) {
      // 128 x 128 tiles run two or three to a CU: a launch is a sequence of rounds of 512 / 768 workgroups,
      // and a last round with few workgroups takes as long as a lone workgroup (measured at two per CU:
      // 501 RoIs of 14 x 14 = 1536 workgroups 0.916 ms, 502 RoIs 1.059 ms).  The pixels of an underfull last round go to a
      // second launch with 128 x 32 tiles: four times the workgroups, a quarter of the time each.
      // The split depends on the launch shape only, and both variants add an output's products
      // in the same order (chunk, tap, channel pair), so results do not depend on it.  A caller that
      // keeps a second stream busy (flag bit 3) has that stream's workgroups fill the last round;
      // the extra dependent launch then only delays its own stream (measured: 250 vs 241 img/s).
      // Worth it while the last round is at most ~0.6 full (measured at 0.01 .. 0.99); DM_CONV_TAIL=0
      // turns it off (A/B measurements).
      static const int tail_mode = getenv("DM_CONV_TAIL") ? atoi(getenv("DM_CONV_TAIL")) : 1;
      const int MT = dm_ceil_div(a.CoutP, 128), NTiles = dm_ceil_div(a.Q, 128);
      const int wgs = MT * NTiles, cus = dm_num_cus();
      // workgroups per CU: 3 when the staged plane needs one position per thread (the 168-VGPR build
      // of the kernel; 14 x 14 maps), else 2
      const int plane128 = conv_plane(128, H, W);
      const int slots = (plane128 <= 256 ? 3 : 2) * cus;
      // A 128-pixel tile whose plane no build can stage (more than 4 x 256 positions: 1 x 1 maps, a tile of 128 images)
      // while the 32-pixel tile's fits: the whole launch takes the 128 x 32 build, whatever its size -- the answer must
      // not depend on NB.  (Maps wider than 168 fit neither: conv_with_maxpos refuses them.)
      if (plane128 > 4 * 256) return launch_conv<3, 4, 1, 1, 1, 8>(a, st);
      // with a workspace: the 128 x 128 tiles (the efficient build) and as many K splits as fill ONE round of slots
      // (100 RoIs of 14 x 14: 306 tiles x 2 splits on 768 slots; the 128 x 32 tiles without a split: 0.233 ms)
      if (a.ws && wgs < slots) {
        // (the split is DECIDED here, with launch_conv_mp's own cost model, before the tile build is chosen --
        // a launch the model then declined to split used to run the 128 x 128 tiles unsplit instead of the 128 x 32 ones)
        const ConvSplit k = conv_split(conv_chunks(num_srcs, src_channels, 8), true, wgs, slots, a.ws_floats, (long long)NB * Cout * H * W);
        if (k.S >= 2) {
          a.want_split = k.S;
          return launch_conv<3, 2, 2, 2, 2, 8>(a, st);
        }
      }
      if (tail_mode && conv_small_launch(wgs, cus)) return launch_conv<3, 4, 1, 1, 1, 8>(a, st);
      const int full_rounds = wgs / slots;
      const int rem = wgs - full_rounds * slots;
      if (tail_mode && !(relu & 8) && full_rounds >= 1 && rem > 0 && rem * 5 <= 3 * slots) {
        const int n_main = full_rounds * slots / MT;
        const int Q = a.Q;
        a.Q = n_main * 128;
        const int rc_main = launch_conv<3, 2, 2, 2, 2, 8>(a, st);
        if (rc_main != DM_OK) return rc_main;
        a.q_begin = a.Q;
        a.Q = Q;
        return launch_conv<3, 4, 1, 1, 1, 8>(a, st);
      }
      return launch_conv<3, 2, 2, 2, 2, 8>(a, st);
    }
    if (Cout > 32 && Cout <= 36 && !(relu & 2)) return launch_conv<3, 1, 4, 1, 1, 8, 4>(a, st);   // DCN offset convs: 32 + 4
    if (Cout > 32) return launch_conv<3, 1, 4, 2, 1, 8>(a, st);
    return launch_conv<3, 1, 4, 1, 1, 8>(a, st);
  }
  if (Cout > 64) {
    // A launch of few 128 x 128 tiles (the <= 100-RoI inference calls: 25-307 workgroups for 256 CUs) is a chain of K
    // chunks per workgroup, and next to another stream's 3x3 launch -- the two RoI chains of a 100-detection call -- each
    // chunk's 32 MFMAs per wave queue behind the neighbour's.  Up to 1.25 tiles per CU the launch takes 128 couts x 32
    // pixels instead: four times the workgroups, 8 MFMAs per wave and chunk.  Same products in the same order (a
    // 32-channel chunk walks its quad pairs in the order two 16-channel chunks do), so rows do not depend on the launch
    // size (tests/test_ops_gpu.py).  Measured (profiles/r06_infer_notes.txt (5)): 100 / 64 / 32 / 16 detections
    // 1.941 / 1.407 / 0.901 / 0.608 -> 1.879 / 1.360 / 0.884 / 0.584 ms; thresholds 100 / 160 / 320 / 640 / 1300 tiles:
    // 1.923 / 1.896 / 1.879-1.891 / 1.883 / 1.887 at 100 detections; 128 x 64 tiles for the next 320-1300 and 64 x 64 tiles
    // for the 64-cout build: inside the noise, not kept.  DM_CONV1_SMALL_WGS: the threshold in tiles (0: off), for A/B runs.
    static const int small_env = getenv("DM_CONV1_SMALL_WGS") ? atoi(getenv("DM_CONV1_SMALL_WGS")) : -1;
    const int small_wgs = small_env >= 0 ? small_env : (5 * dm_num_cus()) / 4;
    // (the POST builds take the tiles the plain launch of the shape takes: the same products in the same order)
    if (!(relu & 2) && !mask && dm_ceil_div(a.CoutP, 128) * dm_ceil_div(a.Q, 128) <= small_wgs)
      return launch_conv_post<1, 4, 1, 1, 1, 32>(a, st);
    return launch_conv_post<1, 2, 2, 2, 2, 16>(a, st);
  }
  if (Cout > 32) {
    // 64 couts x 128 px as 4 waves of 32 x 64: 0.437 -> 0.379 ms on 576 -> 64 @56^2 x 128 RoIs, 0.098 -> 0.089 ms on
    // 64 -> 64 x 256 (the other tilings tried: docs/HISTORY.md, round 3); one k order per output.
    return launch_conv_post<1, 2, 2, 1, 2, 16>(a, st);
  }
  return launch_conv_post<1, 1, 4, 1, 1, 32>(a, st);
}

extern "C" int dm_conv2d_fwd(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                             int num_srcs, int NB, int H, int W,
                             const float* w_packed, const float* bias, int Cout, int ksize, int relu, float* out,
                             int out_ch_total, int out_ch_offset, dm_stream_t stream) {
  return conv2d_launch(srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, w_packed, bias, Cout, ksize, relu, out,
                       out_ch_total, out_ch_offset, nullptr, stream);
}

// (ABI 20) dm_conv2d_fwd with a caller-owned workspace: launches of few workgroups split their K loop over up to eight
// workgroups per tile (bare sums to the workspace, added in split order by a second kernel: the same bits every run; they
// differ from the unsplit sum in rounding only).  dm_conv2d_splitk_floats: the workspace that lets this shape split as far
// as it wants to (0: the launch would not split).
extern "C" long long dm_conv2d_splitk_floats(int NB, int H, int W, int Cout, int ksize) {
  if (NB <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  const long long px = (long long)NB * H * W;
  // tiles of the smallest configuration the launcher would pick: 128 couts x 32 pixels (3x3, Cout > 64), else >= 64 x 128
  const long long wgs = (long long)dm_ceil_div(Cout, 128) * dm_ceil_div(px, 128);
  // split while the tiles do not fill half a round of three slots per CU; the 3x3 launches of 128 x 128 tiles (two or three
  // workgroups per CU) as far as the slots go, the others as far as the chunk count will let them
  const int Smax = conv_split_max(wgs, 3LL * dm_num_cus());
  if (Smax < 2) return 0;
  return (ksize == 3 && Cout > 64 ? Smax : 8) * px * Cout;
}

extern "C" int dm_conv2d_fwd_ws(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                                int num_srcs, int NB, int H, int W,
                                const float* w_packed, const float* bias, int Cout, int ksize, int relu, float* out,
                                int out_ch_total, int out_ch_offset, float* workspace, long long workspace_floats,
                                dm_stream_t stream) {
  return conv2d_launch(srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, w_packed, bias, Cout, ksize, relu, out,
                       out_ch_total, out_ch_offset, nullptr, stream, workspace, workspace_floats);
}

extern "C" int dm_conv2d_fwd_masked(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                                    int num_srcs, int NB, int H, int W,
                                    const float* w_packed, const float* bias, int Cout, int ksize, int relu, float* out,
                                    int out_ch_total, int out_ch_offset, const float* mask, dm_stream_t stream) {
  if (!mask) return DM_ERR_INVALID_ARG;
  return conv2d_launch(srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, w_packed, bias, Cout, ksize, relu, out,
                       out_ch_total, out_ch_offset, mask, stream);
}

// (K26) out = addend + act(conv1x1(srcs) + bias): dm_conv2d_fwd's launch with the POST epilogue.  addend: the layout of out
// (channels [out_ch_offset, out_ch_offset + Cout) of [NB, out_ch_total, H, W]); it may be out.
extern "C" int dm_conv2d_post_add_fwd(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                                      int num_srcs, int NB, int H, int W, const float* w_packed, const float* bias, int Cout,
                                      int ksize, int relu, const float* addend, float* out, int out_ch_total, int out_ch_offset,
                                      dm_stream_t stream) {
  if (!addend) return DM_ERR_INVALID_ARG;
  return conv2d_launch(srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, w_packed, bias, Cout, ksize, relu, out,
                       out_ch_total, out_ch_offset, nullptr, stream, nullptr, 0, addend);
}

// (K31) out = addend[n, c, iy[y], ix[x]] + act(conv1x1(srcs) + bias): the POST epilogue with the addend gathered from a
// dense [NB, Cout, Hs, Ws] map of its own through two device index tables (FPN's top-down merge inside the lateral conv).
// The launch is the plain launch's, as K26's: same tiles, same products in the same order, one more fp32 add.
extern "C" int dm_conv2d_up_add_fwd(const float* const* srcs, const int* src_channels, const long long* src_batch_strides,
                                    int num_srcs, int NB, int H, int W, const float* w_packed, const float* bias, int Cout,
                                    int ksize, int relu, const float* addend, int Hs, int Ws, const int32_t* iy, const int32_t* ix,
                                    float* out, int out_ch_total, int out_ch_offset, dm_stream_t stream) {
  if (!addend || !iy || !ix || Hs <= 0 || Ws <= 0) return DM_ERR_INVALID_ARG;
  if ((long long)Hs * Ws > 0x7fffffffLL) return DM_ERR_INVALID_ARG;
  const UpAdd up = {Hs, Ws, iy, ix};
  return conv2d_launch(srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, w_packed, bias, Cout, ksize, relu, out,
                       out_ch_total, out_ch_offset, nullptr, stream, nullptr, 0, addend, nullptr, &up);
}

// (added to ABI 28) What dm_conv2d_fwd / _ws / _masked / dm_conv2d_post_add_fwd would launch for these host arguments: the
// launcher itself runs with a recorder and launches nothing (no pointer below is read; the header has the record layout).
extern "C" int dm_conv2d_plan(const int* src_channels, const long long* src_batch_strides, int num_srcs, int NB, int H, int W,
                              int Cout, int ksize, int relu, int out_ch_total, int out_ch_offset, long long workspace_floats,
                              int has_mask, int has_addend, int* records, int max_records) {
  if (!records || max_records < DM_CONV_PLAN_MAX_LAUNCHES || workspace_floats < 0) return DM_ERR_INVALID_ARG;
  if ((has_mask || has_addend) && workspace_floats > 0) return DM_ERR_INVALID_ARG;      // (no entry point takes both)
  if (has_mask && has_addend) return DM_ERR_INVALID_ARG;
  static float dummy[4];
  const float* srcs[DM_MAX_SOURCES] = {dummy, dummy, dummy, dummy};
  ConvPlan plan = {DM_CONV_PLAN_MAX_LAUNCHES};
  const int rc = conv2d_launch(srcs, src_channels, src_batch_strides, num_srcs, NB, H, W, dummy, nullptr, Cout, ksize, relu, dummy,
                               out_ch_total, out_ch_offset, has_mask ? dummy : nullptr, nullptr,
                               workspace_floats > 0 ? dummy : nullptr, workspace_floats, has_addend ? dummy : nullptr, &plan);
  return rc != DM_OK ? rc : plan.copy_to(records);
}

// ---------------------------------------------------------------------------
// K16: ConvTranspose2d(k=2, s=2) = four independent 1x1 GEMMs (one per output
// phase).  Run as ONE 1x1 implicit GEMM with 4*Cout packed output channels and
// a pixel-shuffling epilogue.
extern "C" int dm_deconv_pack_weight(const float* w_iohw, int Cin, int Cout, float* w_packed, dm_stream_t stream) {
  if (!w_iohw || !w_packed || Cin <= 0 || Cout <= 0) return DM_ERR_INVALID_ARG;
  PackArgs p;
  p.w = w_iohw; p.wq = w_packed; p.Cout = Cout; p.Cin = Cin; p.kk = 1; p.flip = 0;
  p.rows = Cin; p.cols = 4 * Cout; p.colsP = dm_conv_packed_cout(4 * Cout);
  p.nsrc = 1;
  for (int s = 0; s < DM_MAX_SOURCES; ++s) p.src_c[s] = 0;
  p.src_c[0] = Cin;
  p.KQ = packed_quads(1, p.src_c);
  p.deconv = 1;
  return run_pack(p, (hipStream_t)stream);
}

// (ABI 28) the bf16x3 layout of the deconv weights (flag bit 4 of dm_deconv2x2_fwd): dm_conv_pack_weight_bf16x3's layout of
// the 4 * Cout packed columns, dm_conv_packed_floats_bf16x3(4 * Cout, 1, 1, &Cin) floats
extern "C" int dm_deconv_pack_weight_bf16x3(const float* w_iohw, int Cin, int Cout, float* w_packed, dm_stream_t stream) {
  if (!w_iohw || !w_packed || Cin <= 0 || Cout <= 0) return DM_ERR_INVALID_ARG;
  PackArgs p;
  p.w = w_iohw; p.wq = w_packed; p.Cout = Cout; p.Cin = Cin; p.kk = 1; p.flip = 0;
  p.rows = Cin; p.cols = 4 * Cout; p.colsP = dm_conv_packed_cout(4 * Cout);
  p.nsrc = 1;
  for (int s = 0; s < DM_MAX_SOURCES; ++s) p.src_c[s] = 0;
  p.src_c[0] = Cin;
  p.KQ = packed_words_bf16x3(1, p.src_c);
  p.deconv = 1;
  return run_pack_bf16x3(p, (hipStream_t)stream);
}

extern "C" int dm_deconv2x2_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                                int Cout, int relu, float* out, dm_stream_t stream) {
  if (!x || !w_packed || !out || NB < 0 || C <= 0 || H <= 0 || W <= 0 || Cout <= 0) return DM_ERR_INVALID_ARG;
  if ((long long)NB * H * W > 0x7fffffffLL) return DM_ERR_INVALID_ARG;
  if (NB == 0) return DM_OK;
  const bool bf16x3 = (relu & 16) != 0;          // (ABI 28) w_packed is dm_deconv_pack_weight_bf16x3's layout
  ConvArgs a;
  const int rc = conv_fill(a, &x, &C, nullptr, 1, NB, H, W, w_packed, bf16x3, bias, 4 * Cout, relu & ~16, out, 0, 0, Cout);
  if (rc != DM_OK) return rc;
  if (bf16x3) return launch_conv<1, 2, 2, 1, 2, 16, 0, 1>(a, (hipStream_t)stream);
  return launch_conv<1, 2, 2, 2, 2, 16>(a, (hipStream_t)stream);
}

// (ABI 26) `count` (1..3) independent single-source 1x1 convolutions (+ bias, + ReLU) in ONE launch: x[i] [NB, Cin[i], H[i], W[i]]
// -> out[i] [NB, Cout[i], H[i], W[i]], weights packed by dm_conv_pack_weight (ksize 1, one source).  Every problem runs the
// 64-cout x 128-pixel build of the kernel, in its own range of the grid: the results are those of dm_conv2d_fwd launches
// that take that build (32 < Cout <= 64) and differ from the 128-cout build's (Cout > 64) in nothing -- both walk K in
// chunks of 16 channels in the same order.
extern "C" int dm_conv1x1_group_fwd(int count, const float* const* x, const int* Cin, const int* H, const int* W, int NB,
                                    const float* const* w_packed, const float* const* bias, const int* Cout, int relu,
                                    float* const* out, dm_stream_t stream) {
  if (count < 1 || count > 3 || !x || !Cin || !H || !W || !w_packed || !bias || !Cout || !out || NB < 0) return DM_ERR_INVALID_ARG;
  if (relu & ~17) return DM_ERR_INVALID_ARG;
  const bool bf16x3 = (relu & 16) != 0;          // (ABI 28) every w_packed[i] is the bf16x3 layout
  if (NB == 0) return DM_OK;
  ConvGroup g;
  for (int i = 0; i < 3; ++i) {
    const int j = i < count ? i : count - 1;          // unused slots repeat the last problem (never selected: end[] stops)
    if (!x[j] || !w_packed[j] || !out[j] || Cin[j] <= 0 || H[j] <= 0 || W[j] <= 0 || Cout[j] <= 0) return DM_ERR_INVALID_ARG;
    if ((long long)NB * H[j] * W[j] > 0x7fffffffLL) return DM_ERR_INVALID_ARG;
    const int rc = conv_fill(g.a[i], &x[j], &Cin[j], nullptr, 1, NB, H[j], W[j], w_packed[j], bf16x3, bias[j], Cout[j], relu & 1,
                             out[j], Cout[j], 0, 0);
    if (rc != DM_OK) return rc;
  }
  if (bf16x3) return launch_group<1, 2, 2, 1, 2, 16, 1>(g, count, ConvSplit(), nullptr, (hipStream_t)stream);
  return launch_group<1, 2, 2, 1, 2, 16>(g, count, ConvSplit(), nullptr, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// (added to ABI 28) Stage-grouped convolutions: the three FCNMaskHeads of Cascade Mask R-CNN read the same RoIs and have
// the same shapes, so each layer runs all three stages in ONE launch (conv_igemm_group_kernel over the concatenated grids).
// Tile build: the one dm_conv2d_fwd picks for a lone problem of this shape (3x3, Cout > 64: 128 x 128 tiles when the K loop
// splits or the grid fills the chip, else 128 x 32 -- decided on the grouped workgroup count; 3x3, Cout <= 64: 64 / 32 x 128;
// 1x1: 128 / 64 / 32 couts x 128 px).  Every exact build of the kernel walks K in the order (chunk, tap, quad pair) and
// every 3x3 build takes 8-channel chunks, so a problem's sums are those of dm_conv2d_fwd whatever tile either launch uses;
// the 1x1 builds take 16- or 32-channel chunks, and a 32-channel chunk walks its quad pairs as two 16-channel chunks do.
// With a K split, chunk c of a problem goes to split c / kchunks exactly as in a lone split launch of the same split count,
// and the splits are added in index order by the same reduction arithmetic.  The 36-cout tail build (the DCN offset
// convolutions: v_mfma_f32_4x4x1 rows) has no grouped form: 32 < Cout <= 36 with ksize 3 is refused.
// shuffle != 0: the grouped deconv 2x2/s2 instead (dm_deconv2x2_fwd's GEMM per problem: 4 * Cout packed columns of a 1x1,
// 128 x 128 tiles, the pixel-shuffling epilogue; no workspace).
static int conv2d_group_launch(int count, const float* const* x, int NB, int H, int W, int Cin, int Cout, int ksize,
                               const float* const* w_packed, const float* const* bias, int relu, float* const* out, int shuffle,
                               float* workspace, long long workspace_floats, dm_stream_t stream, ConvPlan* plan) {
  if (ksize != 1 && ksize != 3) return DM_ERR_INVALID_ARG;
  if (count < 1 || count > 3 || !x || !w_packed || !out || NB < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0)
    return DM_ERR_INVALID_ARG;
  if ((long long)NB * H * W > 0x7fffffffLL) return DM_ERR_INVALID_ARG;
  if (relu & ~(1 | 8 | 16)) return DM_ERR_INVALID_ARG;
  if (relu & 16) return DM_ERR_UNSUPPORTED;        // exact fp32 only: the bf16x3 mode runs the per-stage path
  for (int i = 0; i < count && NB > 0; ++i)        // (NB == 0: empty tensors may have null addresses; nothing is read)
    if (!x[i] || !w_packed[i] || !out[i]) return DM_ERR_INVALID_ARG;
  if (ksize == 3 && Cout > 32 && Cout <= 36) return DM_ERR_UNSUPPORTED;
  if (workspace_floats < 0 || (workspace_floats > 0 && !workspace)) return DM_ERR_INVALID_ARG;
  if (NB == 0) return DM_OK;
  ConvGroup g;
  const int flags = (relu & 1) | (shuffle ? 0 : conv_store_policy(NB, Cout, H, W));
  for (int i = 0; i < 3; ++i) {
    const int j = i < count ? i : count - 1;          // unused slots repeat the last problem (never selected: end[] stops)
    const int rc = conv_fill(g.a[i], &x[j], &Cin, nullptr, 1, NB, H, W, w_packed[j], false, bias ? bias[j] : nullptr,
                             shuffle ? 4 * Cout : Cout, flags, out[j], shuffle ? 0 : Cout, 0, shuffle);
    if (rc != DM_OK) return rc;
    g.a[i].plan = plan;
  }
  hipStream_t st = (hipStream_t)stream;
  if (shuffle) return launch_group<1, 2, 2, 2, 2, 16>(g, count, ConvSplit(), nullptr, st);
  const ConvSplit k = workspace ? group_split(count, NB, H, W, Cin, Cout, ksize, workspace_floats) : ConvSplit();
  if (ksize == 3) {
    if (Cout > 64) {
      const int wgs = count * dm_ceil_div(g.a[0].CoutP, 128) * dm_ceil_div(g.a[0].Q, 128);
      if (k.S < 2 && conv_small_launch(wgs, dm_num_cus())) return launch_group<3, 4, 1, 1, 1, 8>(g, count, ConvSplit(), nullptr, st);
      return launch_group<3, 2, 2, 2, 2, 8>(g, count, k, workspace, st);
    }
    if (Cout > 32) return launch_group<3, 1, 4, 2, 1, 8>(g, count, k, workspace, st);
    return launch_group<3, 1, 4, 1, 1, 8>(g, count, k, workspace, st);
  }
  if (Cout > 64) return launch_group<1, 2, 2, 2, 2, 16>(g, count, ConvSplit(), nullptr, st);
  if (Cout > 32) return launch_group<1, 2, 2, 1, 2, 16>(g, count, ConvSplit(), nullptr, st);
  return launch_group<1, 1, 4, 1, 1, 32>(g, count, ConvSplit(), nullptr, st);
}

extern "C" int dm_conv2d_group_splits(int count, int NB, int H, int W, int Cin, int Cout, int ksize, long long workspace_floats) {
  if (count < 1 || count > 3 || NB < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3)) return -1;
  return group_split(count, NB, H, W, Cin, Cout, ksize, workspace_floats).S;
}

extern "C" long long dm_conv2d_group_splitk_floats(int count, int NB, int H, int W, int Cin, int Cout, int ksize) {
  if (count < 1 || count > 3 || NB <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || ksize != 3) return 0;
  const long long per = (long long)NB * Cout * H * W;
  const int S = group_split(count, NB, H, W, Cin, Cout, ksize, 8LL * count * per).S;
  return S >= 2 ? (long long)S * count * per : 0;
}

extern "C" int dm_conv2d_group_fwd(int count, const float* const* x, int NB, int H, int W, int Cin, int Cout, int ksize,
                                   const float* const* w_packed, const float* const* bias, int relu, float* const* out,
                                   float* workspace, long long workspace_floats, dm_stream_t stream) {
  return conv2d_group_launch(count, x, NB, H, W, Cin, Cout, ksize, w_packed, bias, relu, out, 0, workspace, workspace_floats, stream,
                             nullptr);
}

// (added to ABI 28) What dm_conv2d_group_fwd would launch for these host arguments: dm_conv2d_plan's recorder on the grouped
// launcher, one record per problem (the header has the layout); no pointer below is read.
extern "C" int dm_conv2d_group_plan(int count, int NB, int H, int W, int Cin, int Cout, int ksize, int relu,
                                    long long workspace_floats, int* records, int max_records) {
  if (!records || max_records < DM_CONV_GROUP_PLAN_MAX || workspace_floats < 0) return DM_ERR_INVALID_ARG;
  static float dummy[4];
  const float* in[3] = {dummy, dummy, dummy};
  float* out[3] = {dummy, dummy, dummy};
  ConvPlan plan = {DM_CONV_GROUP_PLAN_MAX};
  const int rc = conv2d_group_launch(count, in, NB, H, W, Cin, Cout, ksize, in, nullptr, relu, out, 0,
                                     workspace_floats > 0 ? dummy : nullptr, workspace_floats, nullptr, &plan);
  return rc != DM_OK ? rc : plan.copy_to(records);
}

// (added to ABI 28) 1 to 3 deconv 2x2/s2 problems of one shape in one launch: dm_deconv2x2_fwd's GEMM per problem, in its
// own range of the grid -- the same build on the same operands, so each output has the bits of its own dm_deconv2x2_fwd.
extern "C" int dm_deconv2x2_group_fwd(int count, const float* const* x, int NB, int C, int H, int W,
                                      const float* const* w_packed, const float* const* bias, int Cout, int relu,
                                      float* const* out, dm_stream_t stream) {
  return conv2d_group_launch(count, x, NB, H, W, C, Cout, 1, w_packed, bias, relu, out, Cout, nullptr, 0, stream, nullptr);
}
