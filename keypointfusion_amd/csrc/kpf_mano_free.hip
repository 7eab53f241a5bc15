// The free-space term of the MANO cloud fit (mano_fit.ManoFitter.silhouette / free_space), one 256-thread workgroup per hand:
//   kpf_depth_silhouette_f32   the observed depth crop -> per pixel the nearest observed pixel, its squared distance, the nearest observed depth of the
//                              3 x 3 neighbourhood, and the observed pixels' count: once per frame
//   kpf_mano_free_space_f32    the fitted vertices against those maps -> the vertex targets of the mesh fits (kpf_mano_fit.hip) with the vertices that lie
//                              outside the silhouette or in front of the observed surface overridden: once per round
// The first works in integers and exact minima; in the second every operation is individually rounded and every sum has a fixed order: the host
// restatements in tests/mano_free_cases.py give the same bits.
#include "kpf_mano_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// The silhouette.  Separable: col[r][c] (LDS, 16-bit) = the observed column of row r nearest to c, the lower one on a tie, -1 in a row without any; then a
// pixel scans the rows outward from its own and stops once (r - r')^2 alone exceeds the best distance.  The order of the definition -- the smallest
// (dist2, r', c') -- is kept by the comparisons: a row ABOVE (r' < r) takes the pixel on a tie (<=: it is lower than every row seen before it), a row below
// only if strictly nearer (<: every row seen before it is lower); within a row only its nearest column can be the minimum.
// ---------------------------------------------------------------------------------------------------------------
constexpr int SIL_MAXPIX = 16384;

struct SilhouetteArgs {
  const float* depth;   // [B][H][W]
  int H, W;
  int *nearest, *dist2;  // [B][H][W]
  float* front;          // [B][H][W]
  int* count;            // [B]
};

__device__ __forceinline__ bool sil_seen(float d) { return isfinite(d) && d > 0.0f; }

__global__ __launch_bounds__(256) void depth_silhouette_kernel(SilhouetteArgs a) {
  __shared__ short col[SIL_MAXPIX];
  __shared__ int total;
  const int b = blockIdx.x, t = threadIdx.x, H = a.H, W = a.W, HW = H * W;
  const float* __restrict__ D = a.depth + (long)b * HW;
  float* __restrict__ front = a.front + (long)b * HW;
  if (t == 0) total = 0;
  __syncthreads();
  int n = 0;
  // the mask and the front map in loops of their own, unrolled: the loads of several pixels are in flight together and wait for no store
#pragma unroll 8
  for (int p = t; p < HW; p += 256) {
    const int r = p / W, c = p - r * W;
    const bool seen = sil_seen(D[p]);
    col[p] = seen ? (short)c : (short)-1;
    n += seen ? 1 : 0;
  }
#pragma unroll 4
  for (int p = t; p < HW; p += 256) {
    const int r = p / W, c = p - r * W;
    float f = INFINITY;  // an observed depth is finite: INFINITY left over means none
    const int r0 = r > 0 ? r - 1 : 0, r1 = r < H - 1 ? r + 1 : H - 1, c0 = c > 0 ? c - 1 : 0, c1 = c < W - 1 ? c + 1 : W - 1;
    for (int rr = r0; rr <= r1; ++rr)
      for (int cc = c0; cc <= c1; ++cc) {
        const float o = D[rr * W + cc];
        if (sil_seen(o)) f = fminf(f, o);
      }
    front[p] = f == INFINITY ? 0.0f : f;
  }
  atomicAdd(&total, n);
  __syncthreads();
  for (int r = t; r < H; r += 256) {  // a row per thread: the nearest observed column at or left of c, then against the nearest at or right of it
    short* row = col + r * W;
    int last = -1;
    for (int c = 0; c < W; ++c) {
      if (row[c] >= 0) last = c;
      row[c] = (short)last;
    }
    int next = -1;
    for (int c = W - 1; c >= 0; --c) {
      const int left = row[c];
      if (left == c) next = c;  // observed itself
      const int pick = left < 0 ? next : (next < 0 ? left : (c - left <= next - c ? left : next));
      row[c] = (short)pick;
    }
  }
  __syncthreads();
  const int seen_total = total;
  if (t == 0) a.count[b] = seen_total;
  for (int p = t; p < HW; p += 256) {
    const int r = p / W, c = p - r * W;
    int best = 0x7fffffff, bn = -1;
    if (seen_total > 0)
      for (int dr = 0; dr < H; ++dr) {
        if (dr * dr > best) break;  // dr <= 16383: the square fits
        const int up = r - dr, dn = r + dr;
        if (up < 0 && dn >= H) break;
        if (up >= 0) {
          const int k = col[up * W + c];
          const int d = dr * dr + (c - k) * (c - k);
          if (k >= 0 && d <= best) {
            best = d;
            bn = up * W + k;
          }
        }
        if (dr > 0 && dn < H) {
          const int k = col[dn * W + c];
          const int d = dr * dr + (c - k) * (c - k);
          if (k >= 0 && d < best) {
            best = d;
            bn = dn * W + k;
          }
        }
      }
    a.nearest[(long)b * HW + p] = bn;
    a.dist2[(long)b * HW + p] = bn >= 0 ? best : -1;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The free-space term.  A thread owns vertices t, t + 256, ...; the projection is the raster's (kpf_mano_surface.hip), the pixel is clamped to the window
// in float, and the maps are read from global memory at that one pixel.  Every operation individually rounded: tests/mano_free_cases.py::free_space_host
// gives the same bits.  The two means: the thread's values in ascending vertex order onto +0, the 64-lane butterfly, the four waves in wave order.
// ---------------------------------------------------------------------------------------------------------------
struct ManoFreeArgs {
  const float *verts, *cam, *M;          // [B][778][3], [B][4], [B][2][3] or null
  int H, W;
  const int *nearest, *dist2;            // [B][H][W]
  const float* front;                    // [B][H][W]
  int slack2;
  float margin, step, lambda_free;
  const float *vt_in, *vw_in, *vn_in;    // [B][778][3], [B][778], [B][778][3], or null
  float *vtarget, *vweight, *vnormal;    // [B][778][3], [B][778], [B][778][3]
  int* kind;                             // [B][778]
  float* stats;                          // [B][4]
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void mano_free_space_kernel(ManoFreeArgs a) {
#pragma clang fp contract(off)
  __shared__ float wsum[4][2];
  __shared__ int wcnt[4][2];
  const int b = blockIdx.x, t = threadIdx.x, H = a.H, W = a.W;
  const long HW = (long)H * W;
  const float fx = a.cam[b * 4 + 0], fy = a.cam[b * 4 + 1], u0 = a.cam[b * 4 + 2], v0 = a.cam[b * 4 + 3];
  float m[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  if (a.M)
    for (int k = 0; k < 6; ++k) m[k] = a.M[b * 6 + k];
  const float det = __fsub_rn(__fmul_rn(m[0], m[4]), __fmul_rn(m[1], m[3]));
  const bool det_ok = det != 0.0f && isfinite(det);
  float s1 = 0.0f, s2 = 0.0f;
  int n1 = 0, n2 = 0;
  for (int v = t; v < NV; v += 256) {
    const long i = (long)b * NV + v;
    const float x = a.verts[i * 3 + 0], y = a.verts[i * 3 + 1], z = a.verts[i * 3 + 2];
    const float U = __fadd_rn(__fdiv_rn(__fmul_rn(x, fx), z), u0), V = __fadd_rn(__fdiv_rn(__fmul_rn(y, fy), z), v0);
    const float sx = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], U), __fmul_rn(m[1], V)), m[2]), 0.5f);
    const float sy = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[3], U), __fmul_rn(m[4], V)), m[5]), 0.5f);
    const bool ok = det_ok && isfinite(x) && isfinite(y) && isfinite(z) && z > 0.0f && sx == sx && sy == sy;
    int kind = 0;
    float tx = 0.f, ty = 0.f, tz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, val1 = 0.f, val2 = 0.f;
    if (ok) {
      // clamped in float: +-inf and 1e9 land on the window's border, and the index below is inside [0, H * W)
      const float cf = fminf(fmaxf(floorf(__fadd_rn(sx, 0.5f)), 0.0f), (float)(W - 1)), rf = fminf(fmaxf(floorf(__fadd_rn(sy, 0.5f)), 0.0f), (float)(H - 1));
      const long p = (long)b * HW + (long)(int)rf * W + (int)cf;
      const int d2 = a.dist2[p];
      if (d2 > a.slack2) {
        const int n = a.nearest[p];
        const int rs = n / W, cs = n - rs * W;
        const float aa = __fsub_rn(__fadd_rn((float)cs, 0.5f), m[2]), bb = __fsub_rn(__fadd_rn((float)rs, 0.5f), m[5]);
        const float u = __fdiv_rn(__fsub_rn(__fmul_rn(m[4], aa), __fmul_rn(m[1], bb)), det);
        const float w = __fdiv_rn(__fsub_rn(__fmul_rn(m[0], bb), __fmul_rn(m[3], aa)), det);
        tx = __fmul_rn(__fdiv_rn(__fsub_rn(u, u0), fx), z);
        ty = __fmul_rn(__fdiv_rn(__fsub_rn(w, v0), fy), z);
        tz = z;
        kind = 1;
        val1 = sqrtf((float)d2);  // the correctly rounded root (see mano_assoc_kernel)
      } else if (d2 == 0) {
        const float f = a.front[p];
        const float zt = __fsub_rn(f, a.margin);
        if (f > 0.0f && z < zt) {
          const float s = __fdiv_rn(zt, z);
          tx = __fmul_rn(x, s);
          ty = __fmul_rn(y, s);
          tz = zt;
          kind = 2;
          val2 = __fsub_rn(f, z);
        }
      }
      if (kind != 0) {
        const float dx = __fsub_rn(tx, x), dy = __fsub_rn(ty, y), dz = __fsub_rn(tz, z);
        const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
        if (!(len > 0.0f && isfinite(len))) {
          kind = 0;
          val1 = 0.0f;
          val2 = 0.0f;
        } else {
          if (len > a.step) {
            const float q = __fdiv_rn(a.step, len);
            tx = __fadd_rn(x, __fmul_rn(dx, q));
            ty = __fadd_rn(y, __fmul_rn(dy, q));
            tz = __fadd_rn(z, __fmul_rn(dz, q));
          }
          nx = __fdiv_rn(dx, len);
          ny = __fdiv_rn(dy, len);
          nz = __fdiv_rn(dz, len);
        }
      }
    }
    if (kind != 0) {
      a.vtarget[i * 3 + 0] = tx; a.vtarget[i * 3 + 1] = ty; a.vtarget[i * 3 + 2] = tz;
      a.vnormal[i * 3 + 0] = nx; a.vnormal[i * 3 + 1] = ny; a.vnormal[i * 3 + 2] = nz;
      a.vweight[i] = a.lambda_free;
    } else {  // the inputs, bit for bit
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        a.vtarget[i * 3 + d] = a.vt_in ? a.vt_in[i * 3 + d] : 0.0f;
        a.vnormal[i * 3 + d] = a.vn_in ? a.vn_in[i * 3 + d] : 0.0f;
      }
      a.vweight[i] = a.vw_in ? a.vw_in[i] : 0.0f;
    }
    a.kind[i] = kind;
    s1 = __fadd_rn(s1, val1);  // + 0 leaves a sum's bits as they are
    s2 = __fadd_rn(s2, val2);
    n1 += kind == 1 ? 1 : 0;
    n2 += kind == 2 ? 1 : 0;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  n1 = wave_sum_int(n1);
  n2 = wave_sum_int(n2);
  if ((t & 63) == 0) {
    wsum[t >> 6][0] = s1; wsum[t >> 6][1] = s2;
    wcnt[t >> 6][0] = n1; wcnt[t >> 6][1] = n2;
  }
  __syncthreads();
  if (t == 0) {
    const float S1 = __fadd_rn(__fadd_rn(__fadd_rn(wsum[0][0], wsum[1][0]), wsum[2][0]), wsum[3][0]);
    const float S2 = __fadd_rn(__fadd_rn(__fadd_rn(wsum[0][1], wsum[1][1]), wsum[2][1]), wsum[3][1]);
    const int N1 = wcnt[0][0] + wcnt[1][0] + wcnt[2][0] + wcnt[3][0], N2 = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
    a.stats[(long)b * 4 + 0] = (float)N1;
    a.stats[(long)b * 4 + 1] = N1 > 0 ? __fdiv_rn(S1, (float)N1) : 0.0f;
    a.stats[(long)b * 4 + 2] = (float)N2;
    a.stats[(long)b * 4 + 3] = N2 > 0 ? __fdiv_rn(S2, (float)N2) : 0.0f;
  }
}

}  // namespace

static bool free_window_ok(int H, int W) { return H >= 1 && W >= 1 && H <= SIL_MAXPIX && W <= SIL_MAXPIX && (long)H * W <= SIL_MAXPIX; }

extern "C" int kpf_depth_silhouette_f32(const float* depth_obs, int H, int W, int* nearest, int* dist2, float* front, int* count, int B, void* stream) {
  const char* name = "kpf_depth_silhouette_f32";
  KPF_REQUIRE(depth_obs && nearest && dist2 && front && count, "%s: null pointer", name);
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  KPF_REQUIRE(free_window_ok(H, W), "%s: bad window H=%d W=%d (1 <= H, W; H * W <= %d)", name, H, W, SIL_MAXPIX);
  SilhouetteArgs a;
  a.depth = depth_obs; a.H = H; a.W = W; a.nearest = nearest; a.dist2 = dist2; a.front = front; a.count = count;
  hipLaunchKernelGGL(depth_silhouette_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

extern "C" int kpf_mano_free_space_f32(const float* verts, const float* cam, const float* M, int H, int W, const int* nearest, const int* dist2,
                                       const float* front, int slack2, float margin, float step, float lambda_free, const float* vert_target_in,
                                       const float* vert_weight_in, const float* vert_normal_in, float* vert_target, float* vert_weight,
                                       float* vert_normal, int* kind, float* stats, int B, void* stream) {
  const char* name = "kpf_mano_free_space_f32";
  KPF_REQUIRE(verts && cam && nearest && dist2 && front && vert_target && vert_weight && vert_normal && kind && stats, "%s: null pointer", name);
  KPF_REQUIRE((vert_target_in == nullptr) == (vert_weight_in == nullptr), "%s: vert_target_in and vert_weight_in go together", name);
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  KPF_REQUIRE(free_window_ok(H, W), "%s: bad window H=%d W=%d (1 <= H, W; H * W <= %d)", name, H, W, SIL_MAXPIX);
  KPF_REQUIRE(slack2 >= 0, "%s: slack2=%d is negative", name, slack2);
  KPF_REQUIRE(margin > 0.f, "%s: margin=%g is neither positive nor +inf", name, margin);
  KPF_REQUIRE(step > 0.f, "%s: step=%g is neither positive nor +inf", name, step);
  KPF_REQUIRE(lambda_free >= 0.f && isfinite(lambda_free), "%s: lambda_free=%g is negative or not finite", name, lambda_free);
  ManoFreeArgs a;
  a.verts = verts; a.cam = cam; a.M = M; a.H = H; a.W = W; a.nearest = nearest; a.dist2 = dist2; a.front = front; a.slack2 = slack2;
  a.margin = margin; a.step = step; a.lambda_free = lambda_free; a.vt_in = vert_target_in; a.vw_in = vert_weight_in; a.vn_in = vert_normal_in;
  a.vtarget = vert_target; a.vweight = vert_weight; a.vnormal = vert_normal; a.kind = kind; a.stats = stats;
  hipLaunchKernelGGL(mano_free_space_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}
