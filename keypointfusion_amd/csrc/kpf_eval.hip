// Device-resident evaluation (keypointfusion_amd/evaluation_gpu.py): what one iteration of the reference's test loop (train.py:326-399) derives from the
// stages' joints, without leaving the device.  Two launches per batch, fixed grids, no host synchronisation, no floating-point atomics:
//
//   kpf_eval_errors_f32   one wave64 per (sample, stage), one lane per joint: the per-joint error in mm (train.py:470-488) and the same error after the
//                         Umeyama similarity alignment of the prediction onto the ground truth (util/generateFeature.py:676-703), both in float64 from the
//                         float32 inputs and rounded ONCE to float32 -> err [2][S][B][Jsel]
//   kpf_eval_accumulate   one workgroup per stage: strictly sequential float64 sums of those float32 values, the reference's per-batch means, and integer
//                         PCK counts against a threshold table
//
// The arithmetic order is part of the interface (include/kpf.h): every cross-lane sum is a 64-lane butterfly over lanes >= J holding +0.0, so a sample's
// result depends on its own joints alone (not on B, the grid or a graph replay); every sum over samples is one sequential chain.  The file is compiled with
// floating-point contraction OFF so that the float64 expressions round like the numpy expressions they restate.
#include "kpf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EVAL_MAX_STAGES = 8;
constexpr int EVAL_MAX_JOINTS = 64;      // one lane per joint
constexpr int EVAL_JACOBI_SWEEPS = 8;    // cyclic Jacobi on a symmetric 3 x 3 converges quadratically: 4-5 sweeps reach float64 rounding, 8 is the fixed count
constexpr int EVAL_ACC_NT = 256;

struct EvalStages {  // the stages' joints, passed to the kernel by value
  const float* p[EVAL_MAX_STAGES];
};

// One Jacobi rotation of the symmetric 3 x 3 `a` that annihilates a[p][q]; the rotation is accumulated into the columns of v.
template <int p, int q>
__host__ __device__ inline void eval_jacobi_rotate(double a[3][3], double v[3][3]) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // the smaller root: |angle| <= pi / 4
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  constexpr int r = 3 - p - q;
  const double arp = a[r][p], arq = a[r][q];
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0;
  a[r][p] = a[p][r] = c * arp - s * arq;
  a[r][q] = a[q][r] = s * arp + c * arq;
  for (int k = 0; k < 3; ++k) {
    const double vp = v[k][p], vq = v[k][q];
    v[k][p] = c * vp - s * vq;
    v[k][q] = s * vp + c * vq;
  }
}

template <int i, int k>
__host__ __device__ inline void eval_sort_swap(double lam[3], double v[3][3]) {  // descending
  if (lam[i] < lam[k]) {
    const double l = lam[i];
    lam[i] = lam[k], lam[k] = l;
    for (int r = 0; r < 3; ++r) {
      const double x = v[r][i];
      v[r][i] = v[r][k], v[r][k] = x;
    }
  }
}

__host__ __device__ inline void eval_matvec(const double H[3][3], const double x[3], double y[3]) {
  for (int i = 0; i < 3; ++i) y[i] = H[i][0] * x[0] + H[i][1] * x[1] + H[i][2] * x[2];
}
__host__ __device__ inline double eval_dot(const double x[3], const double y[3]) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }
__host__ __device__ inline void eval_cross(const double x[3], const double y[3], double z[3]) {
  z[0] = x[1] * y[2] - x[2] * y[1];
  z[1] = x[2] * y[0] - x[0] * y[2];
  z[2] = x[0] * y[1] - x[1] * y[0];
}

// a unit vector orthogonal to the unit vector u (only for a rank-deficient H, where the SVD itself is free to choose)
__host__ __device__ inline void eval_any_orthogonal(const double u[3], double w[3]) {
  const int k = fabs(u[0]) <= fabs(u[1]) ? (fabs(u[0]) <= fabs(u[2]) ? 0 : 2) : (fabs(u[1]) <= fabs(u[2]) ? 1 : 2);  // the axis u leans on least
  const double uk = k == 0 ? u[0] : k == 1 ? u[1] : u[2];
  for (int i = 0; i < 3; ++i) w[i] = (i == k ? 1.0 : 0.0) - uk * u[i];
  const double n = sqrt(eval_dot(w, w));
  for (int i = 0; i < 3; ++i) w[i] /= n;
}

// H = U diag(s) V^T of the 3 x 3 cross-covariance -> R = V diag(1, 1, d) U^T with d = sign det(V U^T), and tr = s1 + s2 + d s3 (Umeyama 1991).
// V: eigenvectors of H^T H by cyclic Jacobi, sorted by eigenvalue, the third replaced by v1 x v2 (det V = +1).  U: u1, u2 = H v1, H v2 orthonormalised,
// u3 = u1 x u2 (det U = +1).  With both determinants +1 the reflection case shows as a NEGATIVE third singular value s3 = u3^T H v3, and
// V diag(1, 1, d) U_svd^T = V U^T: no determinant and no branch.
__host__ __device__ inline void eval_umeyama_rotation(const double H[3][3], double R[3][3], double* tr) {
  double a[3][3], v[3][3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      a[i][k] = H[0][i] * H[0][k] + H[1][i] * H[1][k] + H[2][i] * H[2][k];
      v[i][k] = i == k ? 1.0 : 0.0;
    }
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < i; ++k) a[i][k] = a[k][i];  // exactly symmetric
  for (int sweep = 0; sweep < EVAL_JACOBI_SWEEPS; ++sweep) {
    eval_jacobi_rotate<0, 1>(a, v);
    eval_jacobi_rotate<0, 2>(a, v);
    eval_jacobi_rotate<1, 2>(a, v);
  }
  // the columns of the two largest eigenvalues, largest first (compare-and-swap on values: no dynamically indexed register array)
  double lam[3] = {a[0][0], a[1][1], a[2][2]};
  eval_sort_swap<0, 1>(lam, v);
  eval_sort_swap<1, 2>(lam, v);
  eval_sort_swap<0, 1>(lam, v);
  double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3], w[3];
  for (int k = 0; k < 3; ++k) v1[k] = v[k][0], v2[k] = v[k][1];
  eval_cross(v1, v2, v3);
  eval_matvec(H, v1, u1);
  const double s1 = sqrt(eval_dot(u1, u1));
  if (s1 > 0.0) {
    for (int k = 0; k < 3; ++k) u1[k] /= s1;
  } else {
    u1[0] = 1.0, u1[1] = 0.0, u1[2] = 0.0;  // H == 0: any rotation is optimal, the scale is 0
  }
  eval_matvec(H, v2, w);
  const double p = eval_dot(u1, w);
  for (int k = 0; k < 3; ++k) u2[k] = w[k] - p * u1[k];
  const double n2 = sqrt(eval_dot(u2, u2));
  if (n2 > 0.0) {
    for (int k = 0; k < 3; ++k) u2[k] /= n2;
  } else {
    eval_any_orthogonal(u1, u2);  // rank 1: the rotation about u1 is free
  }
  eval_cross(u1, u2, u3);
  eval_matvec(H, v3, w);
  const double s3 = eval_dot(u3, w);
  eval_matvec(H, v2, w);
  const double s2 = eval_dot(u2, w);
  *tr = s1 + s2 + s3;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) R[i][k] = v1[i] * u1[k] + v2[i] * u2[k] + v3[i] * u3[k];
}

#ifdef __HIPCC__
// fixed tree: 64-lane butterfly, every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ double eval_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64) void eval_errors_kernel(EvalStages st, const float* __restrict__ gt, const float* __restrict__ cube,
                                                         const int* __restrict__ score_index, int B, int J, int Jsel, int S, float* __restrict__ err) {
  const int b = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const bool on = lane < J;
  const float* pred = st.p[s] + (size_t)b * J * 3;
  const float* g = gt + (size_t)b * J * 3;
  double a[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0}, half[3];
  for (int k = 0; k < 3; ++k) half[k] = (double)cube[3 * b + k] / 2.0;
  if (on)
    for (int k = 0; k < 3; ++k) a[k] = (double)pred[3 * lane + k], t[k] = (double)g[3 * lane + k];
  // plain error: |(p - g) * cube / 2|, the crop centre cancels (evaluation.xyz2error)
  double d[3];
  for (int k = 0; k < 3; ++k) d[k] = (a[k] - t[k]) * half[k];
  const float e_plain = (float)sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  // evaluation.similarity_align: centroids, H = A0^T B0 / J, variance of A
  const double n = (double)J;
  double ca[3], cb[3], a0[3], b0[3];
  for (int k = 0; k < 3; ++k) {
    ca[k] = eval_wave_sum(a[k]) / n;
    cb[k] = eval_wave_sum(t[k]) / n;
    a0[k] = on ? a[k] - ca[k] : 0.0;
    b0[k] = on ? t[k] - cb[k] : 0.0;
  }
  double H[3][3], R[3][3], tr;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) H[i][k] = eval_wave_sum(a0[i] * b0[k]) / n;
  const double var = eval_wave_sum(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]) / n;
  eval_umeyama_rotation(H, R, &tr);  // every lane holds the same H: computed redundantly, no broadcast
  const double scale = tr / var;     // 0 / 0 = NaN when every predicted joint is the same point, as in the reference
  for (int k = 0; k < 3; ++k) {
    const double al = scale * (R[k][0] * a0[0] + R[k][1] * a0[1] + R[k][2] * a0[2]) + cb[k];
    d[k] = (al - t[k]) * half[k];
  }
  const float e_pa = (float)sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  // the scored joints, in the order of score_index (a lane index: __shfl reads no memory, whatever the table holds)
  const int src = lane < Jsel ? (score_index ? score_index[lane] : lane) : 0;
  const float o_plain = __shfl(e_plain, src, 64), o_pa = __shfl(e_pa, src, 64);
  if (lane < Jsel) {
    const size_t o = ((size_t)s * B + b) * Jsel + lane;
    err[o] = o_plain;
    err[(size_t)S * B * Jsel + o] = o_pa;
  }
}

// One workgroup per stage.  The stage's errors are staged in LDS, then every output element is owned by one thread that walks the samples in order:
// pck[s][j][t] (integer), sum[s][j] (one float64 chain per joint, continued from the state), and the batch mean (one float64 chain over (b, j), j inner).
__global__ __launch_bounds__(EVAL_ACC_NT) void eval_accumulate_kernel(const float* __restrict__ err, const unsigned char* __restrict__ valid,
                                                                      const double* __restrict__ th, int S, int B, int Jsel, int T,
                                                                      long long* __restrict__ n_samples, long long* __restrict__ n_batches,
                                                                      double* __restrict__ sum_err, double* __restrict__ sum_pa,
                                                                      double* __restrict__ sum_bm, double* __restrict__ sum_bm_pa,
                                                                      long long* __restrict__ pck, long long* __restrict__ pck_pa) {
  extern __shared__ float eval_lds[];  // [2][B][Jsel] float, then [B] valid bytes
  const int s = blockIdx.x, tid = threadIdx.x, BJ = B * Jsel;
  unsigned char* ok = reinterpret_cast<unsigned char*>(eval_lds + 2 * BJ);
  for (int i = tid; i < BJ; i += EVAL_ACC_NT) {
    eval_lds[i] = err[(size_t)s * BJ + i];
    eval_lds[BJ + i] = err[((size_t)S + s) * BJ + i];
  }
  for (int i = tid; i < B; i += EVAL_ACC_NT) ok[i] = valid ? (valid[i] != 0) : 1;
  __syncthreads();
  const int JT = Jsel * T, n_items = 2 * JT + 2 * Jsel + 3;
  for (int it = tid; it < n_items; it += EVAL_ACC_NT) {
    if (it < 2 * JT) {  // PCK counts: (double)err_f32 <= thresholds[t], numpy's comparison on the logged value
      const int which = it / JT, r = it - which * JT, j = r / T;
      const double thr = th[r - j * T];
      const float* e = eval_lds + which * BJ + j;
      long long c = 0;
      for (int b = 0; b < B; ++b) c += (ok[b] && (double)e[b * Jsel] <= thr) ? 1 : 0;
      long long* dst = (which ? pck_pa : pck) + (size_t)s * JT + r;
      *dst += c;
    } else if (it < 2 * JT + 2 * Jsel) {  // per-joint sums, continuing the running sum sample by sample
      const int r = it - 2 * JT, which = r / Jsel, j = r - which * Jsel;
      const float* e = eval_lds + which * BJ + j;
      double* dst = (which ? sum_pa : sum_err) + (size_t)s * Jsel + j;
      double acc = *dst;
      for (int b = 0; b < B; ++b)
        if (ok[b]) acc += (double)e[b * Jsel];
      *dst = acc;
    } else if (it < 2 * JT + 2 * Jsel + 2) {  // the reference's batch mean (train.py:381-397): sum over valid (b, j) in order, divided by the count
      const int which = it - 2 * JT - 2 * Jsel;
      const float* e = eval_lds + which * BJ;
      double acc = 0.0;
      long long nv = 0;
      for (int b = 0; b < B; ++b)
        if (ok[b]) {
          ++nv;
          for (int j = 0; j < Jsel; ++j) acc += (double)e[b * Jsel + j];
        }
      if (nv > 0) (which ? sum_bm_pa : sum_bm)[s] += acc / (double)(nv * Jsel);
    } else if (s == 0) {  // the counters, once per launch
      long long nv = 0;
      for (int b = 0; b < B; ++b) nv += ok[b];
      if (nv > 0) {
        *n_samples += nv;
        *n_batches += 1;
      }
    }
  }
}
// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Mesh evaluation (keypointfusion_amd/evaluation_mesh_gpu.py): kpf_eval_mesh_f32, one 256-thread workgroup per hand, and kpf_eval_mesh_accumulate.
// LDS of one hand, V <= 1024: the ground truth and ONE prediction set as float64 coordinate planes (2 * 3 * V * 8 = 48 KiB), the logged float32 err [V]
// and nn [2][V] (12 KiB) that the counts are taken on, and 4 x 10 doubles of reduction scratch: the plain pass runs, then the aligned set overwrites the
// prediction planes and the same pass runs again.
// ---------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int MESH_NT = 256, MESH_WAVES = MESH_NT / 64;
constexpr int MESH_MAX_V = 1024, MESH_MAX_T = 256, MESH_MAX_TF = 8;  // a thread owns vertices t, t + 256, ...: at most 4

// The fixed tree of every sum over vertices: part[k] = thread t's vertices t, t + 256, ... added in ascending order onto +0.0 (the caller's loop), then the
// 64-lane butterfly, then the four waves' sums in wave order.  Every thread returns with the same bits in part[].
template <int N>
__device__ __forceinline__ void mesh_block_sum(double (&part)[N], double (*scratch)[10]) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double w = eval_wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0) scratch[wave][k] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) part[k] = ((scratch[0][k] + scratch[1][k]) + scratch[2][k]) + scratch[3][k];
  __syncthreads();  // scratch is free again
}

// Nearest vertex of the set (sx, sy, sz) for this thread's vertices of the set (qx, qy, qz): candidates in ascending index, strict <, from +inf.  All lanes
// read candidate j at one address (an LDS broadcast); the thread's NB vertices sit in registers.  A NaN distance never wins.
template <int NB>
__device__ __forceinline__ void mesh_nearest(const double* qx, const double* qy, const double* qz, const double* sx, const double* sy, const double* sz, int V,
                                             float* __restrict__ nn_out, int* __restrict__ idx_out, float* nn_lds) {
  const int tid = threadIdx.x;
  double x[NB], y[NB], z[NB], best[NB];
  int idx[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int v = tid + i * MESH_NT;
    const bool on = v < V;
    x[i] = on ? qx[v] : 0.0, y[i] = on ? qy[v] : 0.0, z[i] = on ? qz[v] : 0.0;
    best[i] = __builtin_inf();
    idx[i] = -1;
  }
  for (int j = 0; j < V; ++j) {
    const double cx = sx[j], cy = sy[j], cz = sz[j];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const double dx = x[i] - cx, dy = y[i] - cy, dz = z[i] - cz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < best[i]) best[i] = d2, idx[i] = j;
    }
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int v = tid + i * MESH_NT;
    if (v < V) {
      const float d = (float)sqrt(best[i]);
      nn_out[v] = d, idx_out[v] = idx[i], nn_lds[v] = d;
    }
  }
}

__device__ __forceinline__ void mesh_nearest_n(int nb, const double* qx, const double* qy, const double* qz, const double* sx, const double* sy,
                                               const double* sz, int V, float* nn_out, int* idx_out, float* nn_lds) {
  switch (nb) {  // ceil(V / 256), the same for every thread
    case 1: mesh_nearest<1>(qx, qy, qz, sx, sy, sz, V, nn_out, idx_out, nn_lds); break;
    case 2: mesh_nearest<2>(qx, qy, qz, sx, sy, sz, V, nn_out, idx_out, nn_lds); break;
    case 3: mesh_nearest<3>(qx, qy, qz, sx, sy, sz, V, nn_out, idx_out, nn_lds); break;
    default: mesh_nearest<4>(qx, qy, qz, sx, sy, sz, V, nn_out, idx_out, nn_lds); break;
  }
}

__global__ __launch_bounds__(MESH_NT) void eval_mesh_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ pred_origin,
                                                            const float* __restrict__ gt_origin, const double* __restrict__ th, int T,
                                                            const double* __restrict__ fth, int Tf, int B, int V, float* __restrict__ err,
                                                            float* __restrict__ nn, int* __restrict__ nn_idx, double* __restrict__ mean_err,
                                                            int* __restrict__ pck_cnt, int* __restrict__ f_cnt) {
  extern __shared__ double mesh_lds[];  // g [3][V], p [3][V] double; then err [V], nn [2][V] float
  __shared__ double scratch[MESH_WAVES][10];
  const int b = blockIdx.x, tid = threadIdx.x, nb = (V + MESH_NT - 1) / MESH_NT;
  double *gx = mesh_lds, *gy = gx + V, *gz = gy + V, *px = gz + V, *py = px + V, *pz = py + V;
  float* e_lds = reinterpret_cast<float*>(pz + V);
  float* n_lds = e_lds + V;
  const float* P = pred + (size_t)b * V * 3;
  const float* G = gt + (size_t)b * V * 3;
  double po[3] = {0.0, 0.0, 0.0}, go[3] = {0.0, 0.0, 0.0};
  if (pred_origin)  // both or neither (checked on the host)
    for (int k = 0; k < 3; ++k) po[k] = (double)pred_origin[3 * b + k], go[k] = (double)gt_origin[3 * b + k];
  for (int v = tid; v < V; v += MESH_NT) {
    px[v] = (double)P[3 * v] - po[0], py[v] = (double)P[3 * v + 1] - po[1], pz[v] = (double)P[3 * v + 2] - po[2];
    gx[v] = (double)G[3 * v] - go[0], gy[v] = (double)G[3 * v + 1] - go[1], gz[v] = (double)G[3 * v + 2] - go[2];
  }
  __syncthreads();
  const size_t BV = (size_t)B * V;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {  // the Umeyama alignment of eval_errors_kernel over the V vertices; the aligned set replaces p
      const double n = (double)V;
      double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int v = tid; v < V; v += MESH_NT) c[0] += px[v], c[1] += py[v], c[2] += pz[v], c[3] += gx[v], c[4] += gy[v], c[5] += gz[v];
      mesh_block_sum(c, scratch);
      for (int k = 0; k < 6; ++k) c[k] = c[k] / n;
      double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int v = tid; v < V; v += MESH_NT) {
        const double a0[3] = {px[v] - c[0], py[v] - c[1], pz[v] - c[2]}, b0[3] = {gx[v] - c[3], gy[v] - c[4], gz[v] - c[5]};
        for (int i = 0; i < 3; ++i)
          for (int k = 0; k < 3; ++k) s[3 * i + k] += a0[i] * b0[k];
        s[9] += a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2];
      }
      mesh_block_sum(s, scratch);
      double H[3][3], R[3][3], tr;
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) H[i][k] = s[3 * i + k] / n;
      const double var = s[9] / n;
      eval_umeyama_rotation(H, R, &tr);  // every thread holds the same H
      const double scale = tr / var;     // 0 / 0 = NaN when every predicted vertex is the same point
      for (int v = tid; v < V; v += MESH_NT) {  // each thread rewrites its own vertices only
        const double a0[3] = {px[v] - c[0], py[v] - c[1], pz[v] - c[2]};
        px[v] = scale * (R[0][0] * a0[0] + R[0][1] * a0[1] + R[0][2] * a0[2]) + c[3];
        py[v] = scale * (R[1][0] * a0[0] + R[1][1] * a0[1] + R[1][2] * a0[2]) + c[4];
        pz[v] = scale * (R[2][0] * a0[0] + R[2][1] * a0[1] + R[2][2] * a0[2]) + c[5];
      }
      __syncthreads();
    }
    // per-vertex error and its mean
    double m[1] = {0.0};
    float* e_out = err + pass * BV + (size_t)b * V;
    for (int v = tid; v < V; v += MESH_NT) {
      const double d0 = px[v] - gx[v], d1 = py[v] - gy[v], d2 = pz[v] - gz[v];
      const float e = (float)sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      e_out[v] = e, e_lds[v] = e;
      m[0] += (double)e;
    }
    mesh_block_sum(m, scratch);
    if (tid == 0) mean_err[(size_t)pass * B + b] = m[0] / (double)V;
    // nearest vertices, both directions
    const size_t o0 = ((size_t)pass * 2 + 0) * BV + (size_t)b * V, o1 = ((size_t)pass * 2 + 1) * BV + (size_t)b * V;
    mesh_nearest_n(nb, px, py, pz, gx, gy, gz, V, nn + o0, nn_idx + o0, n_lds);
    mesh_nearest_n(nb, gx, gy, gz, px, py, pz, V, nn + o1, nn_idx + o1, n_lds + V);
    __syncthreads();
    // counts on the logged values: every count is owned by one thread that walks the vertices (all lanes read one address)
    for (int it = tid; it < T + 2 * Tf; it += MESH_NT) {
      int cnt = 0;
      if (it < T) {
        const double thr = th[it];
        for (int v = 0; v < V; ++v) cnt += ((double)e_lds[v] <= thr) ? 1 : 0;
        pck_cnt[((size_t)pass * B + b) * T + it] = cnt;
      } else {
        const int r = it - T, k = r >> 1, dir = r & 1;
        const double thr = fth[k];
        const float* d = n_lds + dir * V;
        for (int v = 0; v < V; ++v) cnt += ((double)d[v] <= thr) ? 1 : 0;
        f_cnt[(((size_t)pass * B + b) * Tf + k) * 2 + dir] = cnt;
      }
    }
    __syncthreads();  // e_lds / n_lds are rewritten by the next pass
  }
}

// One workgroup; every state element is owned by one thread that walks the samples in ascending order and skips valid == 0.
__global__ __launch_bounds__(MESH_NT) void eval_mesh_accumulate_kernel(const float* __restrict__ err, const double* __restrict__ mean_err,
                                                                       const int* __restrict__ pck_cnt, const int* __restrict__ f_cnt,
                                                                       const unsigned char* __restrict__ valid, int B, int V, int T, int Tf,
                                                                       long long* __restrict__ n_samples, long long* __restrict__ n_batches,
                                                                       double* __restrict__ sum_mean_err, double* __restrict__ sum_vert,
                                                                       long long* __restrict__ pck, double* __restrict__ sum_f) {
  const int n_vert = 2 * V, n_pck = 2 * T, n_f = 2 * Tf * 3, n_items = n_vert + n_pck + n_f + 2 + 1;
  for (int it = threadIdx.x; it < n_items; it += MESH_NT) {
    if (it < n_vert) {  // sum_vert [2][V]
      const int a = it / V, v = it - a * V;
      double acc = sum_vert[it];
      for (int b = 0; b < B; ++b)
        if (!valid || valid[b]) acc += (double)err[((size_t)a * B + b) * V + v];
      sum_vert[it] = acc;
    } else if (it < n_vert + n_pck) {  // pck [2][T]
      const int r = it - n_vert, a = r / T, t = r - a * T;
      long long c = 0;
      for (int b = 0; b < B; ++b)
        if (!valid || valid[b]) c += pck_cnt[((size_t)a * B + b) * T + t];
      pck[r] += c;
    } else if (it < n_vert + n_pck + n_f) {  // sum_f [2][Tf][3]: F, P, R of every sample
      const int r = it - n_vert - n_pck, a = r / (Tf * 3), q = r - a * Tf * 3, k = q / 3, which = q - 3 * k;
      double acc = sum_f[r];
      for (int b = 0; b < B; ++b)
        if (!valid || valid[b]) {
          const int* h = f_cnt + (((size_t)a * B + b) * Tf + k) * 2;
          const double Pr = (double)h[0] / (double)V, Rc = (double)h[1] / (double)V;
          const double F = (Pr + Rc > 0.0) ? 2.0 * Pr * Rc / (Pr + Rc) : 0.0;
          acc += which == 0 ? F : which == 1 ? Pr : Rc;
        }
      sum_f[r] = acc;
    } else if (it < n_vert + n_pck + n_f + 2) {  // sum_mean_err [2]
      const int a = it - n_vert - n_pck - n_f;
      double acc = sum_mean_err[a];
      for (int b = 0; b < B; ++b)
        if (!valid || valid[b]) acc += mean_err[(size_t)a * B + b];
      sum_mean_err[a] = acc;
    } else {  // the counters
      long long nv = 0;
      for (int b = 0; b < B; ++b) nv += (!valid || valid[b]) ? 1 : 0;
      if (nv > 0) {
        *n_samples += nv;
        *n_batches += 1;
      }
    }
  }
}
#endif  // __HIPCC__

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int kpf_eval_errors_f32(const float* const* stages, int S, const float* gt, const float* cube, const int* score_index, int B, int J, int Jsel,
                                   float* err, void* stream) {
  KPF_REQUIRE(stages && gt && cube && err, "kpf_eval_errors_f32: null pointer argument");
  KPF_REQUIRE(S > 0 && S <= EVAL_MAX_STAGES, "kpf_eval_errors_f32: S = %d stages (1 .. %d)", S, EVAL_MAX_STAGES);
  KPF_REQUIRE(J > 0 && J <= EVAL_MAX_JOINTS, "kpf_eval_errors_f32: J = %d joints (1 .. %d: one lane per joint)", J, EVAL_MAX_JOINTS);
  KPF_REQUIRE(B > 0 && (long)B * J < (1L << 30), "kpf_eval_errors_f32: bad shape (B %d, J %d)", B, J);
  KPF_REQUIRE(score_index ? (Jsel > 0 && Jsel <= EVAL_MAX_JOINTS) : Jsel == J, "kpf_eval_errors_f32: Jsel = %d scored joints of J = %d (score_index %s)", Jsel, J,
              score_index ? "given" : "NULL: Jsel must equal J");
  EvalStages st = {};
  for (int s = 0; s < S; ++s) {
    KPF_REQUIRE(stages[s], "kpf_eval_errors_f32: stage %d is a null pointer", s);
    st.p[s] = stages[s];
  }
  hipLaunchKernelGGL(eval_errors_kernel, dim3(B, S), dim3(64), 0, ST(stream), st, gt, cube, score_index, B, J, Jsel, S, err);
  return kpf_check_launch("kpf_eval_errors_f32");
}

extern "C" int kpf_eval_accumulate(const float* err, const unsigned char* valid, const double* thresholds, int S, int B, int Jsel, int T, long long* n_samples,
                                   long long* n_batches, double* sum_err, double* sum_pa, double* sum_batch_mean, double* sum_batch_pa_mean, long long* pck,
                                   long long* pck_pa, void* stream) {
  KPF_REQUIRE(err && thresholds && n_samples && n_batches && sum_err && sum_pa && sum_batch_mean && sum_batch_pa_mean && pck && pck_pa,
              "kpf_eval_accumulate: null pointer argument");
  KPF_REQUIRE(S > 0 && S <= EVAL_MAX_STAGES, "kpf_eval_accumulate: S = %d stages (1 .. %d)", S, EVAL_MAX_STAGES);
  KPF_REQUIRE(B > 0 && Jsel > 0 && Jsel <= EVAL_MAX_JOINTS && T > 0 && T <= 4096, "kpf_eval_accumulate: bad shape (B %d, Jsel %d, T %d)", B, Jsel, T);
  const size_t lds = (size_t)2 * B * Jsel * sizeof(float) + (size_t)B;
  KPF_REQUIRE(lds <= 64 * 1024, "kpf_eval_accumulate: B = %d samples of Jsel = %d joints need %zu bytes of LDS (64 KiB: split the batch)", B, Jsel, lds);
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(S), dim3(EVAL_ACC_NT), lds, ST(stream), err, valid, thresholds, S, B, Jsel, T, n_samples, n_batches, sum_err,
                     sum_pa, sum_batch_mean, sum_batch_pa_mean, pck, pck_pa);
  return kpf_check_launch("kpf_eval_accumulate");
}

extern "C" int kpf_eval_mesh_f32(const float* pred, const float* gt, const float* pred_origin, const float* gt_origin, const double* thresholds, int T,
                                 const double* f_thresholds, int Tf, int B, int V, float* err, float* nn, int* nn_idx, double* mean_err, int* pck_cnt,
                                 int* f_cnt, void* stream) {
  KPF_REQUIRE(pred && gt && thresholds && f_thresholds && err && nn && nn_idx && mean_err && pck_cnt && f_cnt, "kpf_eval_mesh_f32: null pointer argument");
  KPF_REQUIRE((pred_origin != nullptr) == (gt_origin != nullptr), "kpf_eval_mesh_f32: pred_origin and gt_origin are given together or both NULL");
  KPF_REQUIRE(V >= 1 && V <= MESH_MAX_V, "kpf_eval_mesh_f32: V = %d vertices (1 .. %d: two float64 sets in LDS)", V, MESH_MAX_V);
  KPF_REQUIRE(T >= 1 && T <= MESH_MAX_T, "kpf_eval_mesh_f32: T = %d thresholds (1 .. %d)", T, MESH_MAX_T);
  KPF_REQUIRE(Tf >= 1 && Tf <= MESH_MAX_TF, "kpf_eval_mesh_f32: Tf = %d F-score thresholds (1 .. %d)", Tf, MESH_MAX_TF);
  KPF_REQUIRE(B >= 1 && (long)B * V < (1L << 28), "kpf_eval_mesh_f32: bad shape (B %d, V %d)", B, V);
  const size_t lds = (size_t)V * (6 * sizeof(double) + 3 * sizeof(float));  // <= 60 KiB, + 320 bytes static
  hipLaunchKernelGGL(eval_mesh_kernel, dim3(B), dim3(MESH_NT), lds, ST(stream), pred, gt, pred_origin, gt_origin, thresholds, T, f_thresholds, Tf, B, V, err, nn,
                     nn_idx, mean_err, pck_cnt, f_cnt);
  return kpf_check_launch("kpf_eval_mesh_f32");
}

extern "C" int kpf_eval_mesh_accumulate(const float* err, const double* mean_err, const int* pck_cnt, const int* f_cnt, const unsigned char* valid, int B, int V,
                                        int T, int Tf, long long* n_samples, long long* n_batches, double* sum_mean_err, double* sum_vert, long long* pck,
                                        double* sum_f, void* stream) {
  KPF_REQUIRE(err && mean_err && pck_cnt && f_cnt && n_samples && n_batches && sum_mean_err && sum_vert && pck && sum_f,
              "kpf_eval_mesh_accumulate: null pointer argument");
  KPF_REQUIRE(V >= 1 && V <= MESH_MAX_V && T >= 1 && T <= MESH_MAX_T && Tf >= 1 && Tf <= MESH_MAX_TF,
              "kpf_eval_mesh_accumulate: bad shape (V %d of 1 .. %d, T %d of 1 .. %d, Tf %d of 1 .. %d)", V, MESH_MAX_V, T, MESH_MAX_T, Tf, MESH_MAX_TF);
  KPF_REQUIRE(B >= 1 && (long)B * V < (1L << 28), "kpf_eval_mesh_accumulate: bad shape (B %d, V %d)", B, V);
  hipLaunchKernelGGL(eval_mesh_accumulate_kernel, dim3(1), dim3(MESH_NT), 0, ST(stream), err, mean_err, pck_cnt, f_cnt, valid, B, V, T, Tf, n_samples, n_batches,
                     sum_mean_err, sum_vert, pck, sum_f);
  return kpf_check_launch("kpf_eval_mesh_accumulate");
}
