// The surface of the fitted MANO mesh against the depth camera, one 256-thread workgroup per hand (mano_fit.ManoFitter):
//   kpf_mano_assoc_f32     depth points -> nearest vertex, per-vertex centroid and weight: the vertex targets of the mesh fits (kpf_mano_fit.hip)
//   kpf_mano_normals_f32   area-weighted vertex normals of the fitted mesh from the model's faces
//   kpf_mano_assoc_vis_f32, kpf_mano_assoc_vis_mask_f32  the association over the vertices that face the camera (and pass the mask)
//   kpf_mano_raster_f32    the z-buffer render: depth, owning face, self-occluded vertices
// Every operation is individually rounded and every sum has a fixed order: host restatements in tests/ give the same bits.
#include "kpf_mano_dev.h"
#include "kpf_raster_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Association: each depth point's nearest vertex, and per vertex the weighted centroid and summed weight of its points -- the vertex targets of the fit
// above, built without atomics.  One workgroup per hand.  Every operation is individually rounded (no contraction) and every sum runs in ascending index
// order, so that a numpy-fp32 restatement gives the same bits (tests/mano_mesh_cases.py::associate_host).
// ---------------------------------------------------------------------------------------------------------------
constexpr int ASSOC_MAXN = 4096;

struct ManoAssocArgs {
  const float *points, *pweight, *verts;  // [B][N][3], [B][N] or null, [B][778][3]
  float max_dist2;
  int N;
  int* idx;                               // [B][N]
  float *vtarget, *vweight, *stats;       // [B][778][3], [B][778], [B][2]
};

struct ManoAssocLds {
  float v[NC];
  int idx[ASSOC_MAXN];
  float dist[ASSOC_MAXN];  // a matched point's distance to its vertex, mm
};

// Both association kernels, after the points' matches s.idx[N] are in LDS (s: the kernel's own LDS struct, taken by reference so that its reads stay LDS
// reads): this thread's vertices t, t + 256, t + 512, (t + 768) get the weighted centroid and the summed weight of their points.  One pass over the points
// in ascending order serves all of them.
template <class Lds>
__device__ __forceinline__ void mano_assoc_centroids(const Lds& s, const float* P, const float* PW, int N, int b, int t, float* vtarget, float* vweight) {
#pragma clang fp contract(off)
  float W[4] = {0.f, 0.f, 0.f, 0.f}, S[4][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (int n = 0; n < N; ++n) {
    const int i = s.idx[n];
    if (i < 0 || (i & 255) != t) continue;
    const float w = PW ? PW[n] : 1.0f;
    const float px = P[n * 3 + 0], py = P[n * 3 + 1], pz = P[n * 3 + 2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((i >> 8) == k) {
        W[k] = __fadd_rn(W[k], w);
        S[k][0] = __fadd_rn(S[k][0], __fmul_rn(w, px));
        S[k][1] = __fadd_rn(S[k][1], __fmul_rn(w, py));
        S[k][2] = __fadd_rn(S[k][2], __fmul_rn(w, pz));
      }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = t + k * 256;
    if (v >= NV) continue;
    const bool any = W[k] > 0.0f;
    vweight[(long)b * NV + v] = any ? W[k] : 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) vtarget[((long)b * NV + v) * 3 + d] = any ? __fdiv_rn(S[k][d], W[k]) : 0.0f;
  }
}

// The statistics' head (one thread), row = this hand's stats: row[0] = the matched points' count, row[1] = their mean distance to their vertex and, with
// PLANE (the LDS struct then has plane[]), row[2] = to that vertex's tangent plane, each summed in ascending point order
template <bool PLANE, class Lds>
__device__ __forceinline__ void mano_assoc_stats(const Lds& s, int N, float* row) {
#pragma clang fp contract(off)
  float sum = 0.f, psum = 0.f;
  int cnt = 0;
  for (int n = 0; n < N; ++n)
    if (s.idx[n] >= 0) {
      sum = __fadd_rn(sum, s.dist[n]);
      if constexpr (PLANE) psum = __fadd_rn(psum, s.plane[n]);
      ++cnt;
    }
  row[0] = (float)cnt;
  row[1] = cnt > 0 ? __fdiv_rn(sum, (float)cnt) : 0.0f;
  if constexpr (PLANE) row[2] = cnt > 0 ? __fdiv_rn(psum, (float)cnt) : 0.0f;
}

__global__ __launch_bounds__(256) void mano_assoc_kernel(ManoAssocArgs a) {
#pragma clang fp contract(off)
  __shared__ ManoAssocLds s;
  const int b = blockIdx.x, t = threadIdx.x, N = a.N;
  const float* P = a.points + (long)b * N * 3;
  const float* PW = a.pweight ? a.pweight + (long)b * N : nullptr;
  for (int c = t; c < NC; c += 256) s.v[c] = a.verts[(long)b * NC + c];
  __syncthreads();
  for (int n = t; n < N; n += 256) {  // the nearest vertex: ascending v, strict <
    const float px = P[n * 3 + 0], py = P[n * 3 + 1], pz = P[n * 3 + 2];
    const float w = PW ? PW[n] : 1.0f;
    float best = INFINITY;
    int bi = 0;
    for (int v = 0; v < NV; ++v) {
      const float dx = __fsub_rn(px, s.v[v * 3 + 0]), dy = __fsub_rn(py, s.v[v * 3 + 1]), dz = __fsub_rn(pz, s.v[v * 3 + 2]);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      if (d2 < best) {
        best = d2;
        bi = v;
      }
    }
    const bool matched = w > 0.0f && isfinite(px) && isfinite(py) && isfinite(pz) && best <= a.max_dist2;
    s.idx[n] = matched ? bi : -1;
    // sqrtf, not __fsqrt_rn: this toolchain's __fsqrt_rn is the native (approximate) root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, sqrtf is the
    // correctly rounded one -- the one numpy computes
    s.dist[n] = matched ? sqrtf(best) : 0.0f;
    a.idx[(long)b * N + n] = matched ? bi : -1;
  }
  __syncthreads();
  mano_assoc_centroids(s, P, PW, N, b, t, a.vtarget, a.vweight);
  if (t == 255) mano_assoc_stats<false>(s, N, a.stats + (long)b * 2);
}

// ---------------------------------------------------------------------------------------------------------------
// Vertex normals: n_v = sign * normalize(sum over the corners of the faces at v of (v1 - v0) x (v2 - v0)) -- unnormalised face normals, so
// area-weighted.  One workgroup per hand; vertices, faces and face normals in LDS.  A thread owns vertices t, t + 256, ... and scans the faces in ascending
// order: no atomics, and the sum's order is the face order.  Every operation individually rounded, as the association: tests/mano_surface_cases.py::
// normals_host gives the same bits.
// ---------------------------------------------------------------------------------------------------------------
constexpr int NORMALS_MAXF = 2048;

struct ManoNormalsArgs {
  const float* verts;  // [B][778][3]
  const int* faces;    // [F][3]
  int F;
  float sign;
  float* normals;      // [B][778][3]
};

struct ManoNormalsLds {
  float v[NC];
  int f[NORMALS_MAXF * 3];     // a face with an index outside 0..777: its first index is -1
  float fn[NORMALS_MAXF * 3];
};

__global__ __launch_bounds__(256) void mano_normals_kernel(ManoNormalsArgs a) {
#pragma clang fp contract(off)
  __shared__ ManoNormalsLds s;
  const int b = blockIdx.x, t = threadIdx.x, F = a.F;
  for (int c = t; c < NC; c += 256) s.v[c] = a.verts[(long)b * NC + c];
  for (int c = t; c < F * 3; c += 256) s.f[c] = a.faces[c];
  __syncthreads();
  for (int k = t; k < F; k += 256) {
    const int i0 = s.f[k * 3 + 0], i1 = s.f[k * 3 + 1], i2 = s.f[k * 3 + 2];
    const bool in = i0 >= 0 && i0 < NV && i1 >= 0 && i1 < NV && i2 >= 0 && i2 < NV;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (in) {
      const float ax = __fsub_rn(s.v[i1 * 3 + 0], s.v[i0 * 3 + 0]), ay = __fsub_rn(s.v[i1 * 3 + 1], s.v[i0 * 3 + 1]), az = __fsub_rn(s.v[i1 * 3 + 2], s.v[i0 * 3 + 2]);
      const float bx = __fsub_rn(s.v[i2 * 3 + 0], s.v[i0 * 3 + 0]), by = __fsub_rn(s.v[i2 * 3 + 1], s.v[i0 * 3 + 1]), bz = __fsub_rn(s.v[i2 * 3 + 2], s.v[i0 * 3 + 2]);
      n0 = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
      n1 = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
      n2 = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
    }
    s.fn[k * 3 + 0] = n0;
    s.fn[k * 3 + 1] = n1;
    s.fn[k * 3 + 2] = n2;
    if (!in) s.f[k * 3 + 0] = -1;  // skipped below (only this thread has read face k so far)
  }
  __syncthreads();
  float S[4][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};  // vertices t, t + 256, t + 512, (t + 768)
  // eight faces' indices are read before any is looked at (k0 + u < 2048 stays inside s.f; a slot past F holds nothing and is masked), so the 24 LDS reads
  // of a step are in flight together; a hit -- six or so per vertex in the whole scan -- is the only branch
  for (int k0 = 0; k0 < F; k0 += 8) {
    int ix[8][3];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int c = 0; c < 3; ++c) ix[u][c] = s.f[(k0 + u) * 3 + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u;
      const bool live = k < F && ix[u][0] >= 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int i = ix[u][c];
        if (!(live && (i & 255) == t)) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((i >> 8) == q) {
            S[q][0] = __fadd_rn(S[q][0], s.fn[k * 3 + 0]);
            S[q][1] = __fadd_rn(S[q][1], s.fn[k * 3 + 1]);
            S[q][2] = __fadd_rn(S[q][2], s.fn[k * 3 + 2]);
          }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int v = t + q * 256;
    if (v >= NV) continue;
    const float len2 = __fadd_rn(__fadd_rn(__fmul_rn(S[q][0], S[q][0]), __fmul_rn(S[q][1], S[q][1])), __fmul_rn(S[q][2], S[q][2]));
    const float len = sqrtf(len2);  // the correctly rounded root (see mano_assoc_kernel)
    const bool ok = len > 0.0f && isfinite(len);
#pragma unroll
    for (int d = 0; d < 3; ++d) a.normals[((long)b * NV + v) * 3 + d] = ok ? __fmul_rn(a.sign, __fdiv_rn(S[q][d], len)) : 0.0f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Association over the vertices that face the camera: mano_assoc_kernel with a visibility flag per vertex.  The camera is the origin of
// the frame, so vertex v is visible iff its normal is finite, not all-zero and n_v . V_v < -facing_min |V_v|.  The argmin runs over the visible vertices
// only (compacted first, in ascending order); everything else -- gate, weights, centroids, rounding, orders -- is the association's.  stats [B][4]: matched points, their mean distance to their
// vertex, their mean |n_i . (p - V_i)|, the visible vertices.  tests/mano_surface_cases.py::associate_vis_host gives the same bits.
// vmask (kpf_mano_assoc_vis_mask_f32; null: none): a vertex whose entry is 0 is no candidate either -- the z-buffer's self-occlusion.
// ---------------------------------------------------------------------------------------------------------------
struct ManoAssocVisArgs {
  const float *points, *pweight, *verts, *normals;  // [B][N][3], [B][N] or null, [B][778][3], [B][778][3]
  const int* vmask;                                 // [B][778] or null
  float max_dist2, facing_min;
  int N;
  int *idx, *visible;                               // [B][N], [B][778]
  float *vtarget, *vweight, *stats;                 // [B][778][3], [B][778], [B][4]
};

struct ManoAssocVisLds {
  float v[NC], n[NC];
  int vis[NV];
  float cv[NC];             // the visible vertices, compacted in ascending order: the argmin's loop is as long as their number
  int cidx[NV], nvis;       // their indices
  int idx[ASSOC_MAXN];
  float dist[ASSOC_MAXN];   // a matched point's distance to its vertex, mm
  float plane[ASSOC_MAXN];  // and to that vertex's tangent plane
};

__global__ __launch_bounds__(256) void mano_assoc_vis_kernel(ManoAssocVisArgs a) {
#pragma clang fp contract(off)
  __shared__ ManoAssocVisLds s;
  const int b = blockIdx.x, t = threadIdx.x, N = a.N;
  const float* P = a.points + (long)b * N * 3;
  const float* PW = a.pweight ? a.pweight + (long)b * N : nullptr;
  for (int c = t; c < NC; c += 256) {
    s.v[c] = a.verts[(long)b * NC + c];
    s.n[c] = a.normals[(long)b * NC + c];
  }
  __syncthreads();
  for (int v = t; v < NV; v += 256) {
    const float nx = s.n[v * 3 + 0], ny = s.n[v * 3 + 1], nz = s.n[v * 3 + 2];
    const float vx = s.v[v * 3 + 0], vy = s.v[v * 3 + 1], vz = s.v[v * 3 + 2];
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(nx, vx), __fmul_rn(ny, vy)), __fmul_rn(nz, vz));
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz)));
    const bool some = isfinite(nx) && isfinite(ny) && isfinite(nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
    const int vis = (some && dot < -__fmul_rn(a.facing_min, len) && (!a.vmask || a.vmask[(long)b * NV + v] != 0)) ? 1 : 0;
    s.vis[v] = vis;
    a.visible[(long)b * NV + v] = vis;
  }
  __syncthreads();
  if (t < 64) {  // wave 0 compacts the visible vertices, 64 at a time, by a ballot: the order stays ascending
    int count = 0;
    for (int base = 0; base < NV; base += 64) {
      const int v = base + t;
      const bool on = v < NV && s.vis[v] != 0;
      const unsigned long long mask = __ballot(on);
      if (on) {
        const int pos = count + __popcll(mask & ((1ull << t) - 1ull));
        s.cidx[pos] = v;
        s.cv[pos * 3 + 0] = s.v[v * 3 + 0];
        s.cv[pos * 3 + 1] = s.v[v * 3 + 1];
        s.cv[pos * 3 + 2] = s.v[v * 3 + 2];
      }
      count += __popcll(mask);
    }
    if (t == 0) s.nvis = count;
  }
  __syncthreads();
  const int nvis = s.nvis;
  for (int n = t; n < N; n += 256) {  // the nearest visible vertex: ascending v, strict <
    const float px = P[n * 3 + 0], py = P[n * 3 + 1], pz = P[n * 3 + 2];
    const float w = PW ? PW[n] : 1.0f;
    float best = INFINITY;
    int bi = -1;
    for (int i = 0; i < nvis; ++i) {
      const float dx = __fsub_rn(px, s.cv[i * 3 + 0]), dy = __fsub_rn(py, s.cv[i * 3 + 1]), dz = __fsub_rn(pz, s.cv[i * 3 + 2]);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      if (d2 < best) {
        best = d2;
        bi = i;
      }
    }
    if (bi >= 0) bi = s.cidx[bi];
    const bool matched = bi >= 0 && w > 0.0f && isfinite(px) && isfinite(py) && isfinite(pz) && best <= a.max_dist2;
    float pl = 0.0f;
    if (matched) {
      const float dx = __fsub_rn(px, s.v[bi * 3 + 0]), dy = __fsub_rn(py, s.v[bi * 3 + 1]), dz = __fsub_rn(pz, s.v[bi * 3 + 2]);
      pl = fabsf(__fadd_rn(__fadd_rn(__fmul_rn(s.n[bi * 3 + 0], dx), __fmul_rn(s.n[bi * 3 + 1], dy)), __fmul_rn(s.n[bi * 3 + 2], dz)));
    }
    s.idx[n] = matched ? bi : -1;
    s.dist[n] = matched ? sqrtf(best) : 0.0f;
    s.plane[n] = pl;
    a.idx[(long)b * N + n] = matched ? bi : -1;
  }
  __syncthreads();
  mano_assoc_centroids(s, P, PW, N, b, t, a.vtarget, a.vweight);
  if (t == 255) {
    mano_assoc_stats<true>(s, N, a.stats + (long)b * 4);
    a.stats[(long)b * 4 + 3] = (float)nvis;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// z-buffer render of the mesh into the crop's pixel grid: depth, the owning face, the vertices that lie behind another part of the mesh
// along their pixel's ray, and the comparison with an observed depth crop.  One workgroup per hand; the z-buffer is H * W 64-bit words of LDS holding
// (bits(d) << 32) | face, and a face's candidate enters by an integer min: a positive float's bits order as the float does, so the smallest depth wins, among
// equal depths the lowest face, whatever the order the faces arrive in.  A thread owns faces t, t + 256, ...: it walks a pixel box of up to
// RASTER_SMALL pixels itself (kpf_raster_dev.h: the edge rule, shared with the overlay) and queues a larger face, which a whole wave then walks, 8 x 8 pixels at a step (the queue's order does not matter either).
// The faces are read from global memory (at 128 x 128 the buffer alone is 131072 of the 163840 bytes).  There is no near-plane clipping: a face with a vertex at z <= 0 is
// skipped whole.  Every operation individually rounded: tests/mano_raster_cases.py::raster_host gives the same bits.
// ---------------------------------------------------------------------------------------------------------------
constexpr int RASTER_MAXPIX = 16384;

struct ManoRasterArgs {
  const float* verts;      // [B][778][3]
  const int* faces;        // [F][3]
  const float *cam, *M;    // [B][4]: fx, fy, u0, v0; [B][2][3] or null (the identity)
  const float* depth_obs;  // [B][H][W] or null
  int F, H, W;
  float margin;
  float* depth;            // [B][H][W]
  int *face, *occluded;    // [B][H][W], [B][778]
  float* stats;            // [B][4]
};

// the launch's dynamic LDS: zb [HW] 64-bit | sx, sy, iz, z [778] float each | ok [778] int | count [4] int | queue [2048] 16-bit
constexpr size_t raster_lds_bytes(int HW) { return (size_t)HW * 8 + (size_t)NV * 5 * 4 + 16 + (size_t)NORMALS_MAXF * 2; }

__global__ __launch_bounds__(256) void mano_raster_kernel(ManoRasterArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned long long raster_zb[];
  const int b = blockIdx.x, t = threadIdx.x, H = a.H, W = a.W, HW = H * W, F = a.F;
  unsigned long long* zb = raster_zb;
  float* sx = reinterpret_cast<float*>(zb + HW);
  float *sy = sx + NV, *iz = sy + NV, *vz = iz + NV;
  int* ok = reinterpret_cast<int*>(vz + NV);
  int* count = ok + NV;  // covered, observed, both; the length of the queue
  unsigned short* queue = reinterpret_cast<unsigned short*>(count + 4);
  for (int p = t; p < HW; p += 256) zb[p] = RASTER_EMPTY;
  if (t < 4) count[t] = 0;
  {
    const float fx = a.cam[b * 4 + 0], fy = a.cam[b * 4 + 1], u0 = a.cam[b * 4 + 2], v0 = a.cam[b * 4 + 3];
    float m[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    if (a.M)
      for (int k = 0; k < 6; ++k) m[k] = a.M[b * 6 + k];
    for (int v = t; v < NV; v += 256) {
      const float x = a.verts[((long)b * NV + v) * 3 + 0], y = a.verts[((long)b * NV + v) * 3 + 1], z = a.verts[((long)b * NV + v) * 3 + 2];
      const float U = __fadd_rn(__fdiv_rn(__fmul_rn(x, fx), z), u0), V = __fadd_rn(__fdiv_rn(__fmul_rn(y, fy), z), v0);
      sx[v] = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], U), __fmul_rn(m[1], V)), m[2]), 0.5f);
      sy[v] = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[3], U), __fmul_rn(m[4], V)), m[5]), 0.5f);
      iz[v] = __fdiv_rn(1.0f, z);
      vz[v] = z;
      ok[v] = (isfinite(x) && isfinite(y) && isfinite(z) && z > 0.0f) ? 1 : 0;
    }
  }
  __syncthreads();
  for (int k = t; k < F; k += 256) {  // a small face is walked by its thread, a large one is queued (at most F <= 2048 entries)
    RasterFace f;
    if (!f.set(a.faces, k, sx, sy, iz, ok, 0, W - 1, 0, H - 1)) continue;
    if ((f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) > RASTER_SMALL) {
      queue[atomicAdd(&count[3], 1)] = (unsigned short)k;
      continue;
    }
    for (int r = f.y0; r <= f.y1; ++r)
      for (int c = f.x0; c <= f.x1; ++c) raster_min(f, c, r, (unsigned)k, &zb[r * W + c]);
  }
  __syncthreads();
  for (int q = t >> 6; q < count[3]; q += 4) {  // a queued face is walked by one wave, 8 x 8 pixels at a step
    const int k = queue[q];
    RasterFace f;
    f.set(a.faces, k, sx, sy, iz, ok, 0, W - 1, 0, H - 1);
    for (int r = f.y0 + ((t & 63) >> 3); r <= f.y1; r += 8)
      for (int c = f.x0 + (t & 7); c <= f.x1; c += 8) raster_min(f, c, r, (unsigned)k, &zb[r * W + c]);
  }
  __syncthreads();
  for (int v = t; v < NV; v += 256) {  // behind the surface that owns its nearest pixel, by more than the margin
    int occ = 0;
    if (ok[v]) {
      const float c = floorf(__fadd_rn(sx[v], 0.5f)), r = floorf(__fadd_rn(sy[v], 0.5f));
      if (c >= 0.0f && c <= (float)(W - 1) && r >= 0.0f && r <= (float)(H - 1)) {
        const unsigned long long key = zb[(int)r * W + (int)c];
        occ = (key != RASTER_EMPTY && __uint_as_float((unsigned)(key >> 32)) < __fsub_rn(vz[v], a.margin)) ? 1 : 0;
      }
    }
    a.occluded[(long)b * NV + v] = occ;
  }
  __syncthreads();  // the keys are replaced below
  const float* obs = a.depth_obs ? a.depth_obs + (long)b * HW : nullptr;
  int n_cov = 0, n_obs = 0, n_both = 0;
  for (int p = t; p < HW; p += 256) {
    const unsigned long long key = zb[p];
    const bool cov = key != RASTER_EMPTY;
    const float d = cov ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
    a.depth[(long)b * HW + p] = d;
    a.face[(long)b * HW + p] = cov ? (int)(unsigned)key : -1;
    n_cov += cov ? 1 : 0;
    if (obs) {
      const float o = obs[p];
      const bool seen = isfinite(o) && o > 0.0f;
      n_obs += seen ? 1 : 0;
      n_both += (seen && cov) ? 1 : 0;
      zb[p] = (unsigned long long)__float_as_uint((seen && cov) ? fabsf(__fsub_rn(d, o)) : 0.0f);  // + 0 leaves a sum's bits as they are
    }
  }
  atomicAdd(&count[0], n_cov);
  atomicAdd(&count[1], n_obs);
  atomicAdd(&count[2], n_both);
  __syncthreads();
  if (obs) {  // |d - d_obs| summed per row in ascending column order, then over the rows in ascending order
    for (int r = t; r < H; r += 256) {
      float s = 0.0f;
      for (int c = 0; c < W; ++c) s = __fadd_rn(s, __uint_as_float((unsigned)zb[r * W + c]));
      zb[r * W] = (unsigned long long)__float_as_uint(s);  // only this thread reads row r
    }
    __syncthreads();
  }
  if (t == 0) {
    float total = 0.0f;
    if (obs)
      for (int r = 0; r < H; ++r) total = __fadd_rn(total, __uint_as_float((unsigned)zb[r * W]));
    a.stats[(long)b * 4 + 0] = (float)count[0];
    a.stats[(long)b * 4 + 1] = (float)count[1];
    a.stats[(long)b * 4 + 2] = (float)count[2];
    a.stats[(long)b * 4 + 3] = count[2] > 0 ? __fdiv_rn(total, (float)count[2]) : 0.0f;
  }
}

}  // namespace

extern "C" int kpf_mano_assoc_f32(const float* points, const float* point_weight, const float* verts, float max_dist2, int* idx, float* vert_target,
                                  float* vert_weight, float* stats, int B, int N, void* stream) {
  KPF_REQUIRE(points && verts && idx && vert_target && vert_weight && stats, "kpf_mano_assoc_f32: null pointer");
  KPF_REQUIRE(B > 0 && N >= 1 && N <= ASSOC_MAXN, "kpf_mano_assoc_f32: bad shape B=%d N=%d (1 <= N <= %d)", B, N, ASSOC_MAXN);
  KPF_REQUIRE(!(max_dist2 < 0.f) && max_dist2 == max_dist2, "kpf_mano_assoc_f32: max_dist2=%g", max_dist2);
  ManoAssocArgs a;
  a.points = points; a.pweight = point_weight; a.verts = verts; a.max_dist2 = max_dist2; a.N = N;
  a.idx = idx; a.vtarget = vert_target; a.vweight = vert_weight; a.stats = stats;
  hipLaunchKernelGGL(mano_assoc_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch("kpf_mano_assoc_f32");
}

extern "C" int kpf_mano_normals_f32(const float* verts, const int* faces, int F, float sign, float* normals, int B, void* stream) {
  KPF_REQUIRE(verts && faces && normals, "kpf_mano_normals_f32: null pointer");
  KPF_REQUIRE(B > 0 && F >= 1 && F <= NORMALS_MAXF, "kpf_mano_normals_f32: bad shape B=%d F=%d (1 <= F <= %d)", B, F, NORMALS_MAXF);
  KPF_REQUIRE(sign == 1.0f || sign == -1.0f, "kpf_mano_normals_f32: sign=%g is neither +1 nor -1", sign);
  ManoNormalsArgs a;
  a.verts = verts; a.faces = faces; a.F = F; a.sign = sign; a.normals = normals;
  hipLaunchKernelGGL(mano_normals_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch("kpf_mano_normals_f32");
}

// The two entries of the association over the visible vertices: `name` prefixes every refusal; vert_mask is the only difference
static int mano_assoc_vis_launch(const char* name, const float* points, const float* point_weight, const float* verts, const float* normals,
                                 const int* vert_mask, float max_dist2, float facing_min, int* idx, float* vert_target, float* vert_weight, int* visible,
                                 float* stats, int B, int N, void* stream) {
  KPF_REQUIRE(points && verts && normals && idx && vert_target && vert_weight && visible && stats, "%s: null pointer", name);
  KPF_REQUIRE(B > 0 && N >= 1 && N <= ASSOC_MAXN, "%s: bad shape B=%d N=%d (1 <= N <= %d)", name, B, N, ASSOC_MAXN);
  KPF_REQUIRE(!(max_dist2 < 0.f) && max_dist2 == max_dist2, "%s: max_dist2=%g", name, max_dist2);
  KPF_REQUIRE(facing_min >= 0.f && facing_min < 1.f, "%s: facing_min=%g outside [0, 1)", name, facing_min);
  ManoAssocVisArgs a;
  a.points = points; a.pweight = point_weight; a.verts = verts; a.normals = normals; a.vmask = vert_mask; a.max_dist2 = max_dist2;
  a.facing_min = facing_min; a.N = N;
  a.idx = idx; a.visible = visible; a.vtarget = vert_target; a.vweight = vert_weight; a.stats = stats;
  hipLaunchKernelGGL(mano_assoc_vis_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

extern "C" int kpf_mano_assoc_vis_f32(const float* points, const float* point_weight, const float* verts, const float* normals, float max_dist2,
                                      float facing_min, int* idx, float* vert_target, float* vert_weight, int* visible, float* stats, int B, int N,
                                      void* stream) {
  return mano_assoc_vis_launch("kpf_mano_assoc_vis_f32", points, point_weight, verts, normals, nullptr, max_dist2, facing_min, idx, vert_target, vert_weight,
                               visible, stats, B, N, stream);
}

extern "C" int kpf_mano_assoc_vis_mask_f32(const float* points, const float* point_weight, const float* verts, const float* normals, const int* vert_mask,
                                           float max_dist2, float facing_min, int* idx, float* vert_target, float* vert_weight, int* visible, float* stats,
                                           int B, int N, void* stream) {
  return mano_assoc_vis_launch("kpf_mano_assoc_vis_mask_f32", points, point_weight, verts, normals, vert_mask, max_dist2, facing_min, idx, vert_target,
                               vert_weight, visible, stats, B, N, stream);
}

extern "C" int kpf_mano_raster_f32(const float* verts, const int* faces, int F, const float* cam, const float* M, int H, int W, float margin,
                                   const float* depth_obs, float* depth, int* face, int* occluded, float* stats, int B, void* stream) {
  const char* name = "kpf_mano_raster_f32";
  KPF_REQUIRE(verts && faces && cam && depth && face && occluded && stats, "%s: null pointer", name);
  KPF_REQUIRE(B > 0 && F >= 1 && F <= NORMALS_MAXF, "%s: bad shape B=%d F=%d (1 <= F <= %d)", name, B, F, NORMALS_MAXF);
  KPF_REQUIRE(H >= 1 && W >= 1 && H <= RASTER_MAXPIX && W <= RASTER_MAXPIX && (long)H * W <= RASTER_MAXPIX, "%s: bad window H=%d W=%d (1 <= H, W; H * W <= %d)",
              name, H, W, RASTER_MAXPIX);
  KPF_REQUIRE(margin >= 0.f && isfinite(margin), "%s: margin=%g is negative or not finite", name, margin);
  ManoRasterArgs a;
  a.verts = verts; a.faces = faces; a.cam = cam; a.M = M; a.depth_obs = depth_obs; a.F = F; a.H = H; a.W = W; a.margin = margin;
  a.depth = depth; a.face = face; a.occluded = occluded; a.stats = stats;
  const size_t lds = raster_lds_bytes(H * W);
  static std::atomic<bool> lds_opt_in[KPF_MAX_DEVICES];
  if (lds > 64 * 1024 && !kpf_raise_lds_limit(reinterpret_cast<const void*>(&mano_raster_kernel), lds_opt_in)) {
    kpf_set_error("%s: cannot raise the dynamic LDS limit", name);
    return KPF_ELAUNCH;
  }
  hipLaunchKernelGGL(mano_raster_kernel, dim3(B), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}
