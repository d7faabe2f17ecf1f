// K36: CARAFE on whole feature maps, scale 2, merged into the lateral below: FPN_CARAFE's top-down step
//   out = addend + carafe(x, softmax_taps(pixel_shuffle(enc)))[:, :, :OH, :OW]
// (mmdet/models/necks/fpn_carafe.py: tensor_add(laterals[i - 1], upsample(laterals[i])) with slice_as).  The upsampled map
// is never stored and the lateral is read once, by the thread that writes it (so out may BE the addend).
//
// Tile.  A workgroup of 256 threads owns MAP_TH x MAP_TW = 8 x 32 INPUT pixels of one image and one group, one input
// pixel per thread, and a range of the group's channel quads.  A thread builds the four normalised K x K kernels of its
// four output pixels once, in registers (4 K K floats), and then walks its channels in chunks of MAP_CQ = 2 quads (8
// channels: at 3 and 4 quads the K = 5 build spills registers).  A chunk's zero-padded tile with its R = K / 2 halo --
// (8 + 2R) x (32 + 2R) pixels -- sits in LDS, channel-quad interleaved (one float4 = the 4 channels of a quad at one pixel), so one ds_read_b128 feeds 16 FMAs; a row of 32
// lanes reads 512 contiguous bytes, conflict-free in every 16-lane group of the b128 read.  The tile is double buffered:
// the next chunk's global loads are issued into registers before the current chunk's FMAs and written to the other
// buffer after them, one barrier per chunk.  A tap outside the image is a zero of the tile -- never another pixel's value
// times 0 -- so a NaN or an Inf reaches exactly the outputs whose window holds it.  A thread stores two neighbouring
// outputs per row (`pair`: one float2 where OW is even and out and addend are 8-byte aligned, so that the pair is
// aligned in every row; two scalar stores otherwise); the cropped row / column of OH = 2H - 1 / OW = 2W - 1 is neither loaded from the addend nor stored.
//
// Arithmetic of an output (all of it is part of the bits): the maximum over the K K taps in tap order (fmaxf), expf(v -
// max) per tap and their sum in tap order, every weight times 1 / sum; then ONE fmaf chain over the taps in order
// i * K + j starting from 0, and ONE fp32 add of the addend to the finished sum.  Nothing of it depends on NB, on the
// tile a pixel falls into or on the channel split.
//
// Channel split.  At one image the largest map of a 1333 x 800 input (100 x 168) has 13 x 6 = 78 pixel tiles: too few
// workgroups for 256 CUs.  The launcher therefore deals the group's C / group / 4 channel quads over `splits` workgroups
// per tile.  chan_split > 0 forces it (the quads per workgroup are ceil(quads / chan_split)); chan_split = 0 chooses
// among the splits of whole chunks of MAP_CQ quads per workgroup the one with the least rounds x (1 + chunks): `rounds`
// is how many times the grid fills the 2 workgroups per CU the registers allow (dm_num_cus()), `chunks` a workgroup's
// channel chunks and the 1 its softmax, which every split workgroup repeats (100 expf per thread against 400 FMAs per
// channel quad); at equal cost the larger workgroups win.  At 100 x 168 and one image that is 6 workgroups per tile
// (468, one round) where a rule of "at least two per CU" gave 546, a second round for 34 of them.  Channels are
// independent, so a channel's bits do not depend on the split.
#include "common.h"

namespace {

constexpr int MAP_TH = 8, MAP_TW = 32, MAP_CQ = 2;
constexpr int MAP_SOFTMAX_CHUNKS = 1;      // a workgroup's softmax (100 expf, 100 loads per thread) counted as one chunk's work

template <int K>
__global__ __launch_bounds__(256, 2) void carafe_map_kernel(const float* __restrict__ x, const float* __restrict__ enc,
                                                            const float* addend, float* out, int C, int H, int W, int group,
                                                            int OH, int OW, int tiles_x, int tiles_y, int splits, int qps,
                                                            int pair) {
  constexpr int KK = K * K, R = K / 2;
  constexpr int PW = MAP_TW + 2 * R, PH = MAP_TH + 2 * R, PP = PW * PH;
  constexpr int CHUNK = MAP_CQ * PP;                 // float4 slots of one chunk's tile
  constexpr int SLOTS = (CHUNK + 255) / 256;         // ... per thread
  __shared__ __attribute__((aligned(16))) float4 tile[2 * CHUNK];
  int bid = blockIdx.x;
  const int tile_x = bid % tiles_x;
  bid /= tiles_x;
  const int tile_y = bid % tiles_y;
  bid /= tiles_y;
  const int split = bid % splits;
  bid /= splits;
  const int g = bid % group;
  const int n = bid / group;
  const int cpg = C / group;
  const int q0 = split * qps, q1 = min(q0 + qps, cpg / 4);     // this workgroup's quads of the group
  const int tid = threadIdx.x;
  const int ty = tid / MAP_TW, tx = tid % MAP_TW;
  const int y = tile_y * MAP_TH + ty, xx = tile_x * MAP_TW + tx;
  const bool active = y < H && xx < W;
  const int HW = H * W, OHW = OH * OW;

  // ---- staging plan: slot s = (quad of the chunk, padded pixel) -> offset in the chunk's 4 q channel planes, -1 = zero
  int soff[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int s = tid + k * 256;
    const int q = s / PP, p = s - q * PP;
    const int py = p / PW, px = p - py * PW;
    const int gy = tile_y * MAP_TH + py - R, gx = tile_x * MAP_TW + px - R;
    const bool in = s < CHUNK && gy >= 0 && gy < H && gx >= 0 && gx < W;
    soff[k] = in ? q * 4 * HW + gy * W + gx : -1;
  }
  const float* xg = x + ((size_t)n * C + (size_t)g * cpg) * HW;       // the group's first channel plane
  float4 st[SLOTS];
  auto load_chunk = [&](int qc) {
    const int nq = min(MAP_CQ, q1 - qc);
    const float* xb = xg + (size_t)qc * 4 * HW;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (soff[k] >= 0 && (tid + k * 256) / PP < nq) {
        const float* src = xb + soff[k];
        v = make_float4(src[0], src[HW], src[2 * HW], src[3 * HW]);
      }
      st[k] = v;
    }
  };
  auto write_chunk = [&](float4* buf) {
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int s = tid + k * 256;
      if (s < CHUNK) buf[s] = st[k];
    }
  };
  load_chunk(q0);

  // ---- this thread's 4 normalised kernels (pixel_shuffle + softmax of mmcv's kernel_normalizer)
  float wk[4][KK];
  {
    const float* e = enc + ((size_t)n * (group * KK * 4) + (size_t)(g * KK) * 4) * HW + (active ? y * W + xx : 0);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      float mx = -INFINITY;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        wk[sub][kk] = active ? e[(size_t)(kk * 4 + sub) * HW] : 0.f;
        mx = fmaxf(mx, wk[sub][kk]);
      }
      float sum = 0.f;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        wk[sub][kk] = expf(wk[sub][kk] - mx);
        sum += wk[sub][kk];
      }
      const float inv = 1.f / sum;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) wk[sub][kk] *= inv;
    }
  }
  write_chunk(tile);
  __syncthreads();

  const int ox = 2 * xx;
  const bool col1 = ox + 1 < OW;
  const size_t img = ((size_t)n * C + (size_t)g * cpg) * OHW + (size_t)(2 * y) * OW + ox;   // (used by active threads only)
  int b = 0;
  for (int qc = q0; qc < q1; qc += MAP_CQ, b ^= 1) {
    const int nq = min(MAP_CQ, q1 - qc);
    const bool more = qc + MAP_CQ < q1;
    if (more) load_chunk(qc + MAP_CQ);                 // in flight under this chunk's FMAs
    const float4* t0 = tile + b * CHUNK + ty * PW + tx;   // tap (i, j) sits at (ty + i) * PW + tx + j in the padded tile
    for (int q = 0; q < nq; ++q) {
      const size_t o0 = img + (size_t)(qc + q) * 4 * OHW;
      float a[4][4];      // [channel][sub] the lateral's values (0 without an addend)
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) a[ch][sub] = 0.f;
      if (active && addend) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int dy = 0; dy < 2; ++dy) {
            if (2 * y + dy >= OH) continue;
            const float* ap = addend + o0 + (size_t)ch * OHW + dy * OW;
            if (pair) {
              const float2 v = *reinterpret_cast<const float2*>(ap);
              a[ch][dy * 2] = v.x;
              a[ch][dy * 2 + 1] = v.y;
            } else {
              a[ch][dy * 2] = ap[0];
              if (col1) a[ch][dy * 2 + 1] = ap[1];
            }
          }
      }
      float4 acc[4];
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) acc[sub] = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4* tq = t0 + q * PP;
#pragma unroll
      for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float4 v = tq[i * PW + j];
#pragma unroll
          for (int sub = 0; sub < 4; ++sub) {
            const float w = wk[sub][i * K + j];
            acc[sub].x = __builtin_fmaf(w, v.x, acc[sub].x);
            acc[sub].y = __builtin_fmaf(w, v.y, acc[sub].y);
            acc[sub].z = __builtin_fmaf(w, v.z, acc[sub].z);
            acc[sub].w = __builtin_fmaf(w, v.w, acc[sub].w);
          }
        }
      if (active) {
        // output pixel (2y + dy, 2x + dx) = sub dy * 2 + dx: the two dx of a row are neighbours
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          if (2 * y + dy >= OH) continue;
          const float r0[4] = {acc[dy * 2].x, acc[dy * 2].y, acc[dy * 2].z, acc[dy * 2].w};
          const float r1[4] = {acc[dy * 2 + 1].x, acc[dy * 2 + 1].y, acc[dy * 2 + 1].z, acc[dy * 2 + 1].w};
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) {
            float* op = out + o0 + (size_t)ch * OHW + dy * OW;
            // (without an addend the sum itself is stored: 0 + (-0) would be +0)
            const float v0 = addend ? a[ch][dy * 2] + r0[ch] : r0[ch], v1 = addend ? a[ch][dy * 2 + 1] + r1[ch] : r1[ch];
            if (pair) {
              *reinterpret_cast<float2*>(op) = make_float2(v0, v1);
            } else {
              op[0] = v0;
              if (col1) op[1] = v1;
            }
          }
        }
      }
    }
    if (more) write_chunk(tile + (b ^ 1) * CHUNK);
    __syncthreads();
  }
}

// The quads per workgroup and the number of split workgroups for a request (see "Channel split" above).
void map_split(int NB, int group, int qpg, int tiles, int chan_split, int* qps, int* splits) {
  int q;
  if (chan_split > 0) {
    q = dm_ceil_div(qpg, chan_split);
  } else {
    // the split whose workgroups take the fewest rounds of resident slots times the work of one workgroup
    const long long wgs = (long long)NB * group * tiles, slots = 2LL * dm_num_cus();
    long long best = -1;
    q = qpg;
    for (int chunks = dm_ceil_div(qpg, MAP_CQ); chunks >= 1; --chunks) {
      const int qq = chunks * MAP_CQ < qpg ? chunks * MAP_CQ : qpg;
      const long long rounds = (wgs * dm_ceil_div(qpg, qq) + slots - 1) / slots;
      const long long cost = rounds * (MAP_SOFTMAX_CHUNKS + chunks);
      if (best < 0 || cost < best) {      // (ties: the larger workgroups, met first)
        best = cost;
        q = qq;
      }
    }
  }
  *qps = q;
  *splits = dm_ceil_div(qpg, q);
}

}  // namespace

extern "C" int dm_carafe_map_supported(int NB, int C, int H, int W, int up_kernel, int group, int OH, int OW) {
  if (NB < 0 || C <= 0 || H <= 0 || W <= 0 || group <= 0) return 0;
  if (up_kernel != 3 && up_kernel != 5) return 0;
  if (C % group != 0 || (C / group) % 4 != 0) return 0;
  if (OH < 2LL * H - 1 || OH > 2LL * H || OW < 2LL * W - 1 || OW > 2LL * W) return 0;
  const long long lim = 1LL << 31;
  const long long hw = (long long)H * W;
  if (hw >= lim || (long long)OH * OW >= lim) return 0;
  const long long nb = NB > 0 ? NB : 1;
  if (nb * C >= lim || nb * C * hw >= lim || nb * C * ((long long)OH * OW) >= lim) return 0;
  const long long ec = (long long)group * up_kernel * up_kernel * 4;
  if (ec >= lim || nb * ec >= lim || nb * ec * hw >= lim) return 0;
  return 1;
}

extern "C" int dm_carafe_map_fwd(const float* x, const float* enc, int NB, int C, int H, int W, int up_kernel, int group,
                                 const float* addend, int OH, int OW, int chan_split, float* out, dm_stream_t stream) {
  if (NB < 0 || C <= 0 || H <= 0 || W <= 0 || group <= 0 || chan_split < 0) return DM_ERR_INVALID_ARG;
  if (!dm_carafe_map_supported(NB, C, H, W, up_kernel, group, OH, OW)) return DM_ERR_UNSUPPORTED;
  const int qpg = C / group / 4;
  if (chan_split > qpg) return DM_ERR_INVALID_ARG;
  if (NB == 0) return DM_OK;           // (the pointers are not read: an empty tensor's may be null)
  if (!x || !enc || !out) return DM_ERR_INVALID_ARG;
  const int tiles_x = dm_ceil_div(W, MAP_TW), tiles_y = dm_ceil_div(H, MAP_TH);
  int qps = 0, splits = 0;
  map_split(NB, group, qpg, tiles_x * tiles_y, chan_split, &qps, &splits);
  // (NB * group * splits * tiles <= NB * (C / 4) * H * W < 2^31)
  const dim3 grid((unsigned)((long long)NB * group * splits * tiles_x * tiles_y));
  hipStream_t st = (hipStream_t)stream;
  // OW = 2W: (oy * OW + 2 xx) is even, so a pair is 8-byte aligned wherever the tensors are
  const int pair = (OW % 2 == 0 && (uintptr_t)out % 8 == 0 && (uintptr_t)addend % 8 == 0) ? 1 : 0;
  if (up_kernel == 5)
    DM_LAUNCH(carafe_map_kernel<5>, grid, dim3(256), 0, st, x, enc, addend, out, C, H, W, group, OH, OW, tiles_x, tiles_y,
              splits, qps, pair);
  else
    DM_LAUNCH(carafe_map_kernel<3>, grid, dim3(256), 0, st, x, enc, addend, out, C, H, W, group, OH, OW, tiles_x, tiles_y,
              splits, qps, pair);
  return dm_check_launch();
}
