// The hands found in the registered depth frame (keypointfusion_amd/detect.py): the near slab of every connected depth surface, gated by
// its back-projected area, ranked by nearness; and the slots handed to the tracks that have none.  The rule is stated in include/kpf.h.
//
// kpf_detect_hands_u16, six launches for any content, each reading what the launch before it completed (no device-wide barrier, no host readback):
//   detect_tile_kernel        one workgroup per 32 x 32 tile: union-find of the tile in LDS, the tile-local roots written as frame indices
//   detect_seam_kernel        one thread per pixel: the pixels of a tile's first column / row join their left / upper neighbour in global memory
//   detect_flatten_kernel     one thread per pixel: label = find(pixel); the component's pixel count and z_min by integer atomics
//   detect_slab_kernel        one thread per pixel: small components dropped; the near slab's integer sums and bounds by integer atomics
//   detect_candidate_kernel   one thread per pixel: the roots that pass the area gate; the K smallest keys of every 256 pixels
//   detect_select_kernel      one workgroup per frame: K rounds of a minimum over those keys, each above the round before; the slots written
// kpf_detect_assign_f64, one launch: one thread per stored frame hands the untaken slots to the free tracks.
//
// Only integer atomics (32-bit min, max, add; 64-bit add) touch shared words, so every output is the same bits whatever the order of arrival.  find and
// union and their termination arguments are in kpf_detect_uf.h, which also compiles for the host.
#include <math.h>

#include "kpf_common.h"

#include "kpf_box_dev.h"
#include "kpf_detect_uf.h"

namespace {

constexpr int DT_MAXF = 32, DT_MAXPIX = 1 << 24, DT_MAXK = 8, DT_STATS = 5, DT_INFO = 8;
constexpr int DT_TILE = 32, DT_TPIX = DT_TILE * DT_TILE;  // a 32 x 32 tile, four pixels per thread of a 256-thread workgroup
constexpr int DT_BIG = 0x7fffffff;
// the per-root words: [F][7][N] int32 behind the parents, [F][4][N] int64
enum { R_CNT = 0, R_ZMIN, R_SLAB, R_X0, R_Y0, R_X1, R_Y1, R_NI32 };
enum { R_S2 = 0, R_SU, R_SV, R_SD, R_NI64 };

struct DetectArgs {
  const unsigned short* depth;  // [F][H][W]
  int* parent;                  // [F][N]
  int* r32;                     // [F][7][N]
  long long* r64;               // [F][4][N]
  unsigned long long* part;     // [F][nb][K]
  int* labels;                  // [F][N]
  int* stats;                   // [F][5]
  double* boxes;                // [F][K][4]
  int* valid;                   // [F][K]
  double* info;                 // [F][K][8]
  int H, W, N, nb, near, far, step_mm, reach_mm, min_pixels, K;
  float expansion;
  double min_area, max_area;
  float cam[DT_MAXF][4];
};

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }
__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_lsum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_kmin(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = (unsigned long long)__shfl_xor((long long)v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

__device__ __forceinline__ void add_i32(int* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void min_i32(int* p, int v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void max_i32(int* p, int v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_i64(long long* p, long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the counters of a workgroup: one LDS add per wave, one global add per workgroup, none for a zero (as kpf_align.hip)
template <int NC>
__device__ __forceinline__ void block_counters(int* cnt, const int* mine, int* stats_at) {
  const int t = threadIdx.x;
  if ((t & 63) == 0)
    for (int k = 0; k < NC; ++k)
      if (mine[k]) atomicAdd(&cnt[k], mine[k]);
  __syncthreads();
  if (t < NC && cnt[t]) add_i32(stats_at + t, cnt[t]);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 1: the tiles.  grid (tiles_x * tiles_y, F): a frame one pixel wide has 2^19 rows of tiles, more than a grid's y takes.  Local index
// l = ly * 32 + lx orders a tile's pixels as the frame index r * W + c does, so the smallest local index of a tile-local component is its smallest frame index.  Only a tile-local root can become a component's root: their per-root words are cleared
// here, and the frame's counters by the first workgroup (nothing adds to either before launch 3).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_tile_kernel(DetectArgs a) {
  __shared__ int lab[DT_TPIX];
  __shared__ unsigned short dd[DT_TPIX];
  const int tiles_x = (a.W + DT_TILE - 1) / DT_TILE, tile_y = (int)blockIdx.x / tiles_x;
  const int t = threadIdx.x, f = blockIdx.y, x0 = ((int)blockIdx.x - tile_y * tiles_x) * DT_TILE, y0 = tile_y * DT_TILE;
  const unsigned short* depth = a.depth + (long)f * a.N;
  if (blockIdx.x == 0 && t < DT_STATS) a.stats[f * DT_STATS + t] = 0;
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int l = t + 256 * k, y = y0 + (l >> 5), x = x0 + (l & 31);
    const bool in = y < a.H && x < a.W;
    const int d = in ? (int)depth[(long)y * a.W + x] : 0;
    ok[k] = in && kpf_detect_valid(d, a.near, a.far);
    dd[l] = (unsigned short)d;
    lab[l] = l;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int l = t + 256 * k;
    if (!ok[k]) continue;  // (the left and upper neighbours of a pixel inside the frame are inside the frame)
    const int d = dd[l];
    if ((l & 31) > 0 && kpf_detect_joined(d, dd[l - 1], a.near, a.far, a.step_mm)) kpf_uf_union<KPF_UF_WORKGROUP>(lab, l, l - 1);
    if (l >= DT_TILE && kpf_detect_joined(d, dd[l - DT_TILE], a.near, a.far, a.step_mm)) kpf_uf_union<KPF_UF_WORKGROUP>(lab, l, l - DT_TILE);
  }
  __syncthreads();
  int* parent = a.parent + (long)f * a.N;
  int* r32 = a.r32 + (long)f * R_NI32 * a.N;
  long long* r64 = a.r64 + (long)f * R_NI64 * a.N;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int l = t + 256 * k, y = y0 + (l >> 5), x = x0 + (l & 31);
    if (!(y < a.H && x < a.W)) continue;
    const int g = y * a.W + x;
    if (!ok[k]) {
      parent[g] = -1;
      continue;
    }
    const int r = kpf_uf_find<KPF_UF_WORKGROUP>(lab, l);
    parent[g] = (y0 + (r >> 5)) * a.W + x0 + (r & 31);
    if (r == l) {
      r32[(long)R_CNT * a.N + g] = 0;
      r32[(long)R_ZMIN * a.N + g] = DT_BIG;
      r32[(long)R_SLAB * a.N + g] = 0;
      r32[(long)R_X0 * a.N + g] = DT_BIG;
      r32[(long)R_Y0 * a.N + g] = DT_BIG;
      r32[(long)R_X1 * a.N + g] = -1;
      r32[(long)R_Y1 * a.N + g] = -1;
      for (int q = 0; q < R_NI64; ++q) r64[(long)q * a.N + g] = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 2: the seams.  grid (nb, F), one thread per pixel; a pixel in the first column (row) of a tile that is not the frame's first joins its left
// (upper) neighbour when the rule joins them.  Both are valid then, so every index find meets is a valid pixel's.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_seam_kernel(DetectArgs a) {
  const int f = blockIdx.y, p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= a.N) return;
  const int y = p / a.W, x = p - y * a.W;
  const bool sx = x > 0 && (x & (DT_TILE - 1)) == 0, sy = y > 0 && (y & (DT_TILE - 1)) == 0;
  if (!sx && !sy) return;
  const unsigned short* depth = a.depth + (long)f * a.N;
  int* parent = a.parent + (long)f * a.N;
  const int d = depth[p];
  if (sx && kpf_detect_joined(d, depth[p - 1], a.near, a.far, a.step_mm)) kpf_uf_union<KPF_UF_AGENT>(parent, p, p - 1);
  if (sy && kpf_detect_joined(d, depth[p - a.W], a.near, a.far, a.step_mm)) kpf_uf_union<KPF_UF_AGENT>(parent, p, p - a.W);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 3: the flatten pass and the first statistics.  The parents are only read here.  The lanes of a wave that share a root are peeled off together: one
// atomic per (wave, root) and word, not one per pixel -- a hand is tens of thousands of pixels adding to one address.  Every peel retires at least its
// leader, so a wave does at most 64.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_flatten_kernel(DetectArgs a) {
  __shared__ int cnt[2];  // valid pixels, components
  const int t = threadIdx.x, lane = t & 63, f = blockIdx.y, p = (int)blockIdx.x * 256 + t;
  if (t < 2) cnt[t] = 0;
  __syncthreads();
  int* parent = a.parent + (long)f * a.N;
  int* r32 = a.r32 + (long)f * R_NI32 * a.N;
  int root = -1, d = 0;
  if (p < a.N) {
    d = a.depth[(long)f * a.N + p];
    if (parent[p] >= 0) root = kpf_uf_find<KPF_UF_AGENT>(parent, p);
    a.labels[(long)f * a.N + p] = root;
  }
  bool todo = root >= 0;
  for (unsigned long long act = __ballot(todo); act != 0; act = __ballot(todo)) {
    const int leader = __ffsll((long long)act) - 1;
    const int r0 = __shfl(root, leader, 64);
    const bool mine = todo && root == r0;
    const int n = wave_count(mine), zm = wave_imin(mine ? d : DT_BIG);
    if (lane == leader) {
      add_i32(&r32[(long)R_CNT * a.N + r0], n);
      min_i32(&r32[(long)R_ZMIN * a.N + r0], zm);
    }
    todo = todo && !mine;
  }
  const int mine[2] = {wave_count(root >= 0), wave_count(root >= 0 && root == p)};
  block_counters<2>(cnt, mine, a.stats + f * DT_STATS);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 4: components below min_pixels lose their labels; the near slab (d <= z_min + reach_mm) of the others is summed at the root.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_slab_kernel(DetectArgs a) {
  __shared__ int cnt[1];  // components >= min_pixels
  const int t = threadIdx.x, lane = t & 63, f = blockIdx.y, p = (int)blockIdx.x * 256 + t;
  if (t < 1) cnt[t] = 0;
  __syncthreads();
  int* r32 = a.r32 + (long)f * R_NI32 * a.N;
  long long* r64 = a.r64 + (long)f * R_NI64 * a.N;
  int root = -1, d = 0, x = 0, y = 0;
  bool kept_root = false, slab = false;
  if (p < a.N) {
    root = a.labels[(long)f * a.N + p];
    if (root >= 0) {
      d = a.depth[(long)f * a.N + p];
      if (r32[(long)R_CNT * a.N + root] < a.min_pixels) {
        a.labels[(long)f * a.N + p] = -1;
      } else {
        kept_root = root == p;
        slab = d <= r32[(long)R_ZMIN * a.N + root] + a.reach_mm;
        y = p / a.W;
        x = p - y * a.W;
      }
    }
  }
  bool todo = slab;
  for (unsigned long long act = __ballot(todo); act != 0; act = __ballot(todo)) {
    const int leader = __ffsll((long long)act) - 1;
    const int r0 = __shfl(root, leader, 64);
    const bool mine = todo && root == r0;
    const int n = wave_count(mine);
    const long long s2 = wave_lsum(mine ? (long long)d * d : 0ll);
    const int su = wave_isum(mine ? x : 0), sv = wave_isum(mine ? y : 0), sd = wave_isum(mine ? d : 0);  // 64 lanes: below 2^31
    const int lx = wave_imin(mine ? x : DT_BIG), ly = wave_imin(mine ? y : DT_BIG), hx = wave_imax(mine ? x : -1), hy = wave_imax(mine ? y : -1);
    if (lane == leader) {
      add_i32(&r32[(long)R_SLAB * a.N + r0], n);
      min_i32(&r32[(long)R_X0 * a.N + r0], lx);
      min_i32(&r32[(long)R_Y0 * a.N + r0], ly);
      max_i32(&r32[(long)R_X1 * a.N + r0], hx);
      max_i32(&r32[(long)R_Y1 * a.N + r0], hy);
      add_i64(&r64[(long)R_S2 * a.N + r0], s2);
      add_i64(&r64[(long)R_SU * a.N + r0], (long long)su);
      add_i64(&r64[(long)R_SV * a.N + r0], (long long)sv);
      add_i64(&r64[(long)R_SD * a.N + r0], (long long)sd);
    }
    todo = todo && !mine;
  }
  const int mine[1] = {wave_count(kept_root)};
  block_counters<1>(cnt, mine, a.stats + f * DT_STATS + 2);
}

__device__ __forceinline__ double detect_area(long long s2, const float* cam) {
#pragma clang fp contract(off)
  return (double)s2 / ((double)cam[0] * (double)cam[1]);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 5: the candidates.  A kept root whose slab area lies in the gate; of the candidates among a workgroup's 256 pixels the K smallest keys go to
// part[f][workgroup][0..K), sorted, the rest NOKEY.  A key's place is the number of smaller keys: no arrival order enters.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_candidate_kernel(DetectArgs a) {
  __shared__ unsigned long long keys[256];
  __shared__ unsigned long long best[DT_MAXK];
  __shared__ int cnt[1];
  const int t = threadIdx.x, f = blockIdx.y, p = (int)blockIdx.x * 256 + t;
  if (t < 1) cnt[t] = 0;
  if (t < DT_MAXK) best[t] = KPF_DETECT_NOKEY;
  unsigned long long key = KPF_DETECT_NOKEY;
  if (p < a.N && a.labels[(long)f * a.N + p] == p) {
    const double area = detect_area(a.r64[((long)f * R_NI64 + R_S2) * a.N + p], a.cam[f]);
    if (area >= a.min_area && area <= a.max_area) key = kpf_detect_key(a.r32[((long)f * R_NI32 + R_ZMIN) * a.N + p], p);
  }
  keys[t] = key;
  __syncthreads();
  if (key != KPF_DETECT_NOKEY) {
    int rank = 0;
    for (int i = 0; i < 256; ++i) rank += keys[i] < key;
    if (rank < a.K) best[rank] = key;
  }
  const int mine[1] = {wave_count(key != KPF_DETECT_NOKEY)};
  block_counters<1>(cnt, mine, a.stats + f * DT_STATS + 3);  // (its barrier also orders `best`)
  if (t < a.K) a.part[((long)f * a.nb + blockIdx.x) * a.K + t] = best[t];
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 6: the selection and the slots.  grid F.  Round k takes the smallest key above round k - 1's: the K smallest keys in order, for any number of
// candidates.  Then thread k writes slot k.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_select_kernel(DetectArgs a) {
  __shared__ unsigned long long wmin[4];
  __shared__ unsigned long long win[DT_MAXK];
  const int t = threadIdx.x, f = blockIdx.x;
  const unsigned long long* part = a.part + (long)f * a.nb * a.K;
  const long m = (long)a.nb * a.K;
  unsigned long long prev = 0;
  for (int k = 0; k < a.K; ++k) {
    unsigned long long b = KPF_DETECT_NOKEY;
    for (long i = t; i < m; i += 256) {
      const unsigned long long q = part[i];
      if (q < b && (k == 0 || q > prev)) b = q;
    }
    b = wave_kmin(b);
    if ((t & 63) == 0) wmin[t >> 6] = b;
    __syncthreads();
    unsigned long long w = wmin[0];
    for (int i = 1; i < 4; ++i) w = wmin[i] < w ? wmin[i] : w;
    if (t == 0) win[k] = w;
    prev = w;  // NOKEY once the candidates are used up: nothing is above it
    __syncthreads();
  }
  if (t >= a.K) return;
  const unsigned long long key = win[t];
  double box[4] = {0.0, 0.0, 0.0, 0.0}, info[DT_INFO] = {-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int ok = 0;
  if (key != KPF_DETECT_NOKEY) {
#pragma clang fp contract(off)
    const int label = kpf_detect_key_label(key);
    const int* r32 = a.r32 + (long)f * R_NI32 * a.N;
    const long long* r64 = a.r64 + (long)f * R_NI64 * a.N;
    const int slab = r32[(long)R_SLAB * a.N + label];
    info[0] = (double)label;
    info[1] = (double)kpf_detect_key_zmin(key);
    info[2] = (double)r32[(long)R_CNT * a.N + label];
    info[3] = (double)slab;
    info[4] = detect_area(r64[(long)R_S2 * a.N + label], a.cam[f]);
    info[5] = (double)r64[(long)R_SU * a.N + label] / (double)slab;
    info[6] = (double)r64[(long)R_SV * a.N + label] / (double)slab;
    info[7] = (double)r64[(long)R_SD * a.N + label] / (double)slab;
    ok = kpf_next_box((float)r32[(long)R_X0 * a.N + label], (float)r32[(long)R_X1 * a.N + label], (float)r32[(long)R_Y0 * a.N + label],
                      (float)r32[(long)R_Y1 * a.N + label], a.expansion, a.W, a.H, box)
             ? 1
             : 0;
  }
  const long s = (long)f * a.K + t;
  for (int i = 0; i < 4; ++i) a.boxes[s * 4 + i] = box[i];
  for (int i = 0; i < DT_INFO; ++i) a.info[s * DT_INFO + i] = info[i];
  a.valid[s] = ok;
  const int emitted = wave_count(key != KPF_DETECT_NOKEY);  // (K <= 8: the slots' threads are lanes of the first wave)
  if (t == 0) a.stats[f * DT_STATS + 4] = emitted;
}

// ---------------------------------------------------------------------------------------------------------------
// The assignment.  One thread per stored frame; a track belongs to one frame, so no two threads touch one track.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void detect_assign_kernel(const double* __restrict__ boxes, const int* __restrict__ valid, const double* __restrict__ info,
                                                           int F, int K, int frame_w, int frame_h, const int* __restrict__ frame_index, int B,
                                                           int reseed_after, double* __restrict__ bbox, int* __restrict__ lost, int* __restrict__ seeded,
                                                           int* __restrict__ reseeded) {
  const int f = threadIdx.x;
  if (f >= F) return;
  unsigned open = 0;  // bit k: slot k is valid and no live track of this frame stands on it
  for (int k = 0; k < K; ++k) open |= valid[f * K + k] != 0 ? 1u << k : 0u;
  for (int b = 0; b < B; ++b) {
    if (frame_index[b] != f || seeded[b] == 0 || lost[b] >= reseed_after) continue;
    const double x = bbox[4 * b], y = bbox[4 * b + 1], w = bbox[4 * b + 2], h = bbox[4 * b + 3];
    for (int k = 0; k < K; ++k) {
      const double u = info[((long)f * K + k) * DT_INFO + 5], v = info[((long)f * K + k) * DT_INFO + 6];
      if (x <= u && u < x + w && y <= v && v < y + h) open &= ~(1u << k);
    }
  }
  int next = 0;
  for (int b = 0; b < B; ++b) {
    if (frame_index[b] != f) continue;
    int got = 0;
    if (seeded[b] == 0 || lost[b] >= reseed_after) {
      while (next < K && !((open >> next) & 1u)) ++next;
      if (next < K) {
        for (int i = 0; i < 4; ++i) bbox[4 * b + i] = boxes[((long)f * K + next) * 4 + i];
        lost[b] = 0;
        seeded[b] = 1;
        got = 1;
        ++next;
      } else if (seeded[b] == 0) {  // nothing to hold yet: the whole frame, a defined input of prepare
        bbox[4 * b] = 0.0;
        bbox[4 * b + 1] = 0.0;
        bbox[4 * b + 2] = (double)frame_w;
        bbox[4 * b + 3] = (double)frame_h;
      }
    }
    reseeded[b] = got;
  }
}

}  // namespace

extern "C" long kpf_detect_ws64_words(int F, int H, int W, int K) {
  if (F < 1 || H < 1 || W < 1 || K < 1 || K > DT_MAXK || (long)H * W > DT_MAXPIX) return -1;
  const long n = (long)H * W;
  return (long)F * (R_NI64 * n + ((n + 255) / 256) * K);
}

extern "C" int kpf_detect_hands_u16(const unsigned short* depth, int F, int H, int W, const float* cam, int near, int far, int step_mm, int reach_mm,
                                    int min_pixels, double min_area_mm2, double max_area_mm2, float expansion, int K, int* ws32, long long* ws64, double* boxes,
                                    int* valid, double* info, int* labels, int* stats, void* stream) {
  const char* name = "kpf_detect_hands_u16";
  KPF_REQUIRE(depth && cam && ws32 && ws64 && boxes && valid && info && labels && stats, "%s: null pointer", name);
  KPF_REQUIRE(F >= 1 && F <= DT_MAXF && H >= 1 && W >= 1, "%s: bad shape F=%d H=%d W=%d (1 <= F <= %d; 1 <= H, W)", name, F, H, W, DT_MAXF);
  KPF_REQUIRE((long)H * W <= DT_MAXPIX, "%s: a frame of %d x %d holds more than 2^24 pixels", name, H, W);
  KPF_REQUIRE(K >= 1 && K <= DT_MAXK, "%s: slots=%d outside 1..%d", name, K, DT_MAXK);
  KPF_REQUIRE(near >= 0 && near <= far && far <= 65535, "%s: near=%d, far=%d (0 <= near <= far <= 65535)", name, near, far);
  KPF_REQUIRE(step_mm >= 0 && step_mm <= 65535 && reach_mm >= 0 && reach_mm <= 65535, "%s: step_mm=%d, reach_mm=%d outside 0..65535", name, step_mm, reach_mm);
  KPF_REQUIRE(min_pixels >= 1, "%s: min_pixels=%d < 1", name, min_pixels);
  KPF_REQUIRE(isfinite(min_area_mm2) && isfinite(max_area_mm2) && min_area_mm2 >= 0.0 && min_area_mm2 <= max_area_mm2,
              "%s: area gate [%g, %g] (finite, 0 <= min <= max)", name, min_area_mm2, max_area_mm2);
  KPF_REQUIRE(expansion > 0.0f && expansion < 1e6f, "%s: expansion %g (a positive factor)", name, (double)expansion);
  for (int f = 0; f < F; ++f) {
    const float* k = cam + 4 * f;
    KPF_REQUIRE(isfinite(k[0]) && isfinite(k[1]) && isfinite(k[2]) && isfinite(k[3]), "%s: cam[%d] holds a value that is not finite", name, f);
    KPF_REQUIRE(k[0] > 0.f && k[1] > 0.f, "%s: cam[%d] holds a focal length <= 0 (%g, %g)", name, f, k[0], k[1]);
  }
  KPF_REQUIRE((reinterpret_cast<uintptr_t>(depth) & 1u) == 0 && (reinterpret_cast<uintptr_t>(ws32) & 3u) == 0 && (reinterpret_cast<uintptr_t>(labels) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(valid) & 3u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3u) == 0 && (reinterpret_cast<uintptr_t>(ws64) & 7u) == 0 &&
                  (reinterpret_cast<uintptr_t>(boxes) & 7u) == 0 && (reinterpret_cast<uintptr_t>(info) & 7u) == 0,
              "%s: a pointer is not aligned to its element size", name);
  DetectArgs a;
  const int n = H * W;
  a.depth = depth;
  a.parent = ws32;
  a.r32 = ws32 + (long)F * n;
  a.r64 = ws64;
  a.nb = (n + 255) / 256;
  a.part = reinterpret_cast<unsigned long long*>(ws64 + (long)F * R_NI64 * n);
  a.labels = labels; a.stats = stats; a.boxes = boxes; a.valid = valid; a.info = info;
  a.H = H; a.W = W; a.N = n; a.near = near; a.far = far; a.step_mm = step_mm; a.reach_mm = reach_mm; a.min_pixels = min_pixels; a.K = K;
  a.expansion = expansion; a.min_area = min_area_mm2; a.max_area = max_area_mm2;
  for (int i = 0; i < DT_MAXF * 4; ++i) a.cam[i / 4][i % 4] = i < 4 * F ? cam[i] : 0.f;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_pixel((unsigned)a.nb, (unsigned)F), wg(256);
  hipLaunchKernelGGL(detect_tile_kernel, dim3((unsigned)(((W + DT_TILE - 1) / DT_TILE) * ((H + DT_TILE - 1) / DT_TILE)), (unsigned)F), wg, 0, s, a);
  hipLaunchKernelGGL(detect_seam_kernel, per_pixel, wg, 0, s, a);
  hipLaunchKernelGGL(detect_flatten_kernel, per_pixel, wg, 0, s, a);
  hipLaunchKernelGGL(detect_slab_kernel, per_pixel, wg, 0, s, a);
  hipLaunchKernelGGL(detect_candidate_kernel, per_pixel, wg, 0, s, a);
  hipLaunchKernelGGL(detect_select_kernel, dim3((unsigned)F), wg, 0, s, a);
  return kpf_check_launch(name);
}

extern "C" int kpf_detect_assign_f64(const double* boxes, const int* valid, const double* info, int F, int K, int frame_w, int frame_h, const int* frame_index,
                                     int B, int reseed_after, double* bbox, int* lost, int* seeded, int* reseeded, void* stream) {
  const char* name = "kpf_detect_assign_f64";
  KPF_REQUIRE(boxes && valid && info && frame_index && bbox && lost && seeded && reseeded, "%s: null pointer", name);
  KPF_REQUIRE(F >= 1 && F <= DT_MAXF && K >= 1 && K <= DT_MAXK && B >= 1 && frame_w >= 1 && frame_h >= 1,
              "%s: bad shape F=%d K=%d B=%d frame %d x %d (1 <= F <= %d, 1 <= K <= %d)", name, F, K, B, frame_w, frame_h, DT_MAXF, DT_MAXK);
  KPF_REQUIRE(reseed_after >= 1, "%s: reseed_after=%d < 1", name, reseed_after);
  hipLaunchKernelGGL(detect_assign_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), boxes, valid, info, F, K, frame_w, frame_h, frame_index,
                     B, reseed_after, bbox, lost, seeded, reseeded);
  return kpf_check_launch(name);
}
