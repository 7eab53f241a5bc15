// The MANO fits, one 256-thread workgroup per sample, every iteration inside the one launch (mano_fit.ManoFitter):
//   kpf_mano_fit_f32       Adam on pose / shape / translation against 21 target joints
//   kpf_mano_fit_mesh_f32  the same fit with a vertex term (778 weighted vertex targets): the second instantiation of the fit kernel
//   kpf_mano_fit_gn_f32    the joint fit by damped Gauss-Newton: forward-mode Jacobian, normal matrix and Cholesky solve in LDS
//   kpf_mano_fit_mesh_gn_f32  the Gauss-Newton fit with the vertex term: 2334 more rows, J^T J on the fp32 MFMA
//   kpf_mano_fit_mesh_gn_plane_f32  the Gauss-Newton mesh fit with one point-to-plane row per vertex: the second instantiation of that kernel
// The fits share the layer's stage functions (kpf_mano_dev.h) and the pieces marked "written once" below.
// Every reduction has a fixed order (wave butterflies, then a fixed sum over the four waves) and there are no atomics: a replay is bit-identical and a
// sample's bits do not depend on B or on its position in the batch.
#include "kpf_mano_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Fit: Adam on (pose_aa 48, betas 10, trans 3) of one sample against 21 target joints; every iteration inside the launch, state and moments in LDS.
// ---------------------------------------------------------------------------------------------------------------
struct ManoFitIo {                 // what every fit kernel reads and writes alike (filled by mano_fit_host)
  const float *target, *weight;    // [B][21][3] mm or null (no joint carries weight), [B][21] >= 0 or null (= ones)
  float *pose, *betas, *trans;     // the state, [B][48], [B][10], [B][3]: updated in place
  float *verts, *joints, *rotmat;  // [B][778][3] or null, [B][21][3], [B][16][9] or null
  float* residual;
  int* status;
  int res_ld;                      // 2: residual [B][2] (joints before / after); 4: [B][4], the vertex distances before / after in columns 2, 3
};

struct ManoFitArgs {
  ManoFitIo io;
  const float *vtarget, *vweight;  // [B][778][3] mm, [B][778] >= 0: the vertex term (the instantiation with VT only)
  ManoModel m;
  kpf_mano_fit_cfg c;
  float lambda_verts;
};

struct ManoFitLds {
  float P[61], M1[61], M2[61], Gd[61];  // parameters (pose 0..47, betas 48..57, trans 58..60), Adam's moments, the gradient
  float Y[21][3], W[21];                // targets (selected to 0 where the weight is 0) and weights, in the MODEL's joint order: row joint_map[i] is target i
  float Jm[21][3];                      // model joints in joints3d order, mm, without the translation
  float gJ[21][3];                      // d L / d (model joint), mm
  float tip[5][3];
  float sw;
  int status;
  float red[4][4];                      // the four waves' partial sums of a reduction over the vertices
  float sv;                             // the sum of the vertex weights
  double redd[4][3];                    // the same for the one reduction in double (init_trans from the vertices)
};

// Sum of up to four per-thread values over the workgroup in a fixed order: the xor butterfly inside each wave, then the four waves' partials in wave order
// (as mano_backward_lds reduces d G2).  All 256 threads; out[i] is valid in every thread.  Barriers before the partials are overwritten and after they are written.
template <int N>
__device__ __forceinline__ void mano_block_sum(ManoFitLds& f, int t, const float* in, float* out) {
  const int wave = t >> 6, lane = t & 63;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float sum = wave_sum(in[i]);
    if (lane == 0) f.red[wave][i] = sum;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = ((f.red[0][i] + f.red[1][i]) + f.red[2][i]) + f.red[3][i];
}

// The same for three doubles
__device__ __forceinline__ void mano_block_sum3d(ManoFitLds& f, int t, const double* in, double* out) {
  const int wave = t >> 6, lane = t & 63;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = in[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) f.redd[wave][i] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = ((f.redd[0][i] + f.redd[1][i]) + f.redd[2][i]) + f.redd[3][i];
}

// Vertex v of the state in s, in mm without the translation, into vm[v]: lanes over vertices, as the final skinning
__device__ __forceinline__ void mano_fit_skin_all(const ManoModel& m, const ManoLds& s, float* vm, int t) {
  for (int v = t; v < NV; v += 256) {
    float o[3];
    mano_skin_vertex(m, s, v, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) vm[v * 3 + r] = o[r] * 1000.0f;
  }
}

// P -> the model's 21 joints (f.Jm); s holds the forward state afterwards.  With the vertex term every vertex is skinned (vm[778][3], mm, without the
// translation) and the tips are read from there; without it only the five tips are.  Ends with a barrier.
template <bool VT>
__device__ __forceinline__ void mano_fit_eval(const ManoModel& m, ManoLds& s, ManoFitLds& f, float* vm, int t) {
  if (t < 10) s.beta[t] = f.P[48 + t];
  if (t < NJ) {
    float aa[3] = {f.P[t * 3 + 0], f.P[t * 3 + 1], f.P[t * 3 + 2]};
    if (t > 0)
      for (int i = 0; i < 3; ++i) aa[i] = m.hands_mean[(t - 1) * 3 + i] + aa[i];
    mano_set_rotation(s, t, aa);
  }
  mano_blend_chain(m, s, t);
  if constexpr (VT) {
    mano_fit_skin_all(m, s, vm, t);
  } else {
    if (t < 5) mano_skin_vertex(m, s, kManoTip[t], f.tip[t]);
  }
  __syncthreads();
  if (t < 21 * 3) {
    const int i = t / 3, d = t - i * 3;
    const int src = kManoOut[i];
    if constexpr (VT) {
      f.Jm[i][d] = src < NJ ? s.G[src][d * 4 + 3] * 1000.0f : vm[kManoTip[src - NJ] * 3 + d];
    } else {
      const float v = src < NJ ? s.G[src][d * 4 + 3] : f.tip[src - NJ][d];
      f.Jm[i][d] = v * 1000.0f;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float mano_fit_residual(const ManoFitLds& f) {  // mean weighted joint distance, mm (one thread)
  if (!(f.sw > 0.0f)) return 0.0f;
  float sum = 0.f;
  for (int h = 0; h < 21; ++h) {
    if (!(f.W[h] > 0.0f)) continue;
    const float r0 = f.Jm[h][0] + f.P[58] - f.Y[h][0], r1 = f.Jm[h][1] + f.P[59] - f.Y[h][1], r2 = f.Jm[h][2] + f.P[60] - f.Y[h][2];
    sum = fmaf(f.W[h], sqrtf(r0 * r0 + r1 * r1 + r2 * r2), sum);
  }
  return sum / f.sw;
}

// The vertex term's share of one thread: vertices t, t + 256, ... of vm (mm, without the translation) against the targets and weights in global memory (they
// stay in L2; LDS holds none of them).  A target under weight 0 is selected out, never multiplied.
//   mano_vert_weights   -> in[0] = sum of the positive weights, in[1] = how many targets under a positive weight are not finite
//   mano_vert_offset    -> in[d] = sum u_v (c_v - V_v)[d], in double           (init_trans of a vertex-only fit)
//   mano_vert_distance  -> sum u_v |V_v + t - c_v|                             (the residual's numerator)
//   mano_vert_gradient  -> vm[v] = d L / d (posed vertex v, metres) = 2 lambda u_v (V_v + t - c_v) / sv * 1000, every slot written exactly once,
//                          in[d] = this thread's share of d L / d t
__device__ __forceinline__ void mano_vert_weights(const float* c, const float* u, int t, float* in) {
  in[0] = in[1] = 0.f;
  for (int v = t; v < NV; v += 256) {
    const float w = u[v];
    if (!(w > 0.0f)) continue;
    in[0] += w;
    if (!(isfinite(c[v * 3 + 0]) && isfinite(c[v * 3 + 1]) && isfinite(c[v * 3 + 2]))) in[1] += 1.0f;
  }
}

__device__ __forceinline__ void mano_vert_offset(const float* c, const float* u, const float* vm, int t, double* in) {
  in[0] = in[1] = in[2] = 0.0;
  for (int v = t; v < NV; v += 256) {
    const float w = u[v];
    if (!(w > 0.0f)) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) in[d] = fma((double)w, (double)c[v * 3 + d] - (double)vm[v * 3 + d], in[d]);
  }
}

__device__ __forceinline__ float mano_vert_distance(const float* c, const float* u, const float* vm, const float* tr, int t) {
  float sum = 0.f;
  for (int v = t; v < NV; v += 256) {
    const float w = u[v];
    if (!(w > 0.0f)) continue;
    const float r0 = vm[v * 3 + 0] + tr[0] - c[v * 3 + 0], r1 = vm[v * 3 + 1] + tr[1] - c[v * 3 + 1], r2 = vm[v * 3 + 2] + tr[2] - c[v * 3 + 2];
    sum = fmaf(w, sqrtf(r0 * r0 + r1 * r1 + r2 * r2), sum);
  }
  return sum;
}

__device__ __forceinline__ void mano_vert_gradient(const float* c, const float* u, float* vm, const float* tr, float lambda, float sv, int t, float* in) {
  in[0] = in[1] = in[2] = 0.f;
  for (int v = t; v < NV; v += 256) {
    const float w = u[v];
    const bool on = w > 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float gv = on ? 2.0f * lambda * w * (vm[v * 3 + d] + tr[d] - c[v * 3 + d]) / sv : 0.0f;
      vm[v * 3 + d] = gv * 1000.0f;
      in[d] += gv;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// What the three fit kernels (Adam, joint Gauss-Newton, mesh Gauss-Newton) do alike, written once ("The fit kernels' shared pieces").
// ---------------------------------------------------------------------------------------------------------------

// The state into f.P (threads 0..60) and the joint targets and weights into f.Y / f.W in the MODEL's order (threads 64..84): every sum over the joints
// runs in that order, so a permuted joint_map with equally permuted targets gives the same bits.  inv: null, or [21] <- the target row of model joint h.
__device__ __forceinline__ void mano_fit_load(const ManoFitIo& io, const int* joint_map, ManoFitLds& f, int* inv, int b, int t) {
  if (t < 48) f.P[t] = io.pose[(long)b * 48 + t];
  else if (t < 58) f.P[t] = io.betas[(long)b * 10 + (t - 48)];
  else if (t < 61) f.P[t] = io.trans[(long)b * 3 + (t - 58)];
  if (t >= 64 && t < 64 + 21) {
    const int i = t - 64, h = joint_map[i];
    const float w = io.target ? (io.weight ? io.weight[(long)b * 21 + i] : 1.0f) : 0.0f;  // no joint targets (the mesh entries allow it): every joint weight is 0
    f.W[h] = w;
    if (inv) inv[h] = i;
    for (int d = 0; d < 3; ++d) f.Y[h][d] = w > 0.0f ? io.target[((long)b * 21 + i) * 3 + d] : 0.0f;  // a target of weight 0 is selected out, not multiplied
  }
}

// f.sw, f.sv and f.status by thread 0.  vstat: null (no vertex term), or the sum of the vertex weights and the count of non-finite vertex targets (or
// normals) under a positive weight; bit 1 then needs both weight sums to be 0.  All 256 threads; barriers at entry and exit.
__device__ __forceinline__ void mano_fit_status(ManoFitLds& f, const float* vstat, int t) {
  __syncthreads();
  if (t == 0) {
    float sw = 0.f;
    int st = 0;
    for (int i = 0; i < 21; ++i) {
      if (!(f.W[i] > 0.0f)) continue;
      sw += f.W[i];
      if (!(isfinite(f.Y[i][0]) && isfinite(f.Y[i][1]) && isfinite(f.Y[i][2]))) st |= 2;
    }
    if (vstat && vstat[1] > 0.0f) st |= 2;
    if (!(sw > 0.0f) && !(vstat && vstat[0] > 0.0f)) st |= 1;
    f.sw = sw;
    f.sv = vstat ? vstat[0] : 0.0f;
    f.status = st;
  }
  __syncthreads();
}

// init_trans, "before iteration 1": the translation <- the weighted mean offset of the targets from the model at t = 0 (f.Jm, vm: after mano_fit_eval).
// From the joints when they carry weight, otherwise from the vertices (c, u, vm: the vertex targets, weights and skinned vertices; null without a vertex
// term); summed in double and rounded once: at half a metre one float ulp is 6e-5 mm, a sum of 21 such offsets in float is off by about that, and an error
// of t is the same for every vertex -- it does not average out of the pose gradient as a vertex's own rounding does, and was the largest term of the first
// step's pose error.  FLOAT_SUM: the Adam joint fit's rule, older than that finding and kept for its bits.  All 256 threads; ends with a barrier.
template <bool FLOAT_SUM>
__device__ __forceinline__ void mano_fit_init_trans(ManoFitLds& f, const float* c, const float* u, const float* vm, int t) {
  if constexpr (FLOAT_SUM) {
    if (t < 3) {
      float sum = 0.f;
      for (int i = 0; i < 21; ++i)
        if (f.W[i] > 0.0f) sum = fmaf(f.W[i], f.Y[i][t] - f.Jm[i][t], sum);
      f.P[58 + t] = sum / f.sw;
    }
  } else if (!c || f.sw > 0.0f) {
    if (t < 3) {
      double sum = 0.0, den = 0.0;
      for (int i = 0; i < 21; ++i)
        if (f.W[i] > 0.0f) {
          sum = fma((double)f.W[i], (double)f.Y[i][t] - (double)f.Jm[i][t], sum);
          den += (double)f.W[i];
        }
      f.P[58 + t] = (float)(sum / den);
    }
  } else {  // no joint carries weight: the translation comes from the vertices
    double in[3], off[3];
    mano_vert_offset(c, u, vm, t, in);
    mano_block_sum3d(f, t, in, off);
    if (t < 3) f.P[58 + t] = (float)((t == 0 ? off[0] : (t == 1 ? off[1] : off[2])) / (double)f.sv);
  }
  __syncthreads();
}

// The epilogue but for the vertices (each kernel writes those from where it holds them): the state if the fit ran (ok), the joints in target order with the
// translation added, rodrigues(pose_aa[j]) without hands_mean
__device__ __forceinline__ void mano_fit_store(const ManoFitIo& io, const int* joint_map, const ManoFitLds& f, bool ok, int b, int t) {
  if (ok) {
    if (t < 48) io.pose[(long)b * 48 + t] = f.P[t];
    else if (t < 58) io.betas[(long)b * 10 + (t - 48)] = f.P[t];
    else if (t < 61) io.trans[(long)b * 3 + (t - 58)] = f.P[t];
  }
  if (t < 63) {
    const int i = t / 3, d = t - i * 3;
    io.joints[((long)b * 21 + i) * 3 + d] = f.Jm[joint_map[i]][d] + f.P[58 + d];
  }
  if (io.rotmat && t >= 64 && t < 64 + NJ) {
    float R[9];
    rodrigues(&f.P[(t - 64) * 3], R);
    for (int i = 0; i < 9; ++i) io.rotmat[((long)b * NJ + (t - 64)) * 9 + i] = R[i];
  }
}

// The vertices of the state in s, re-skinned, in mm with the translation added (the Adam and the joint Gauss-Newton kernels; o * 1000 + t contracts to an fma)
__device__ __forceinline__ void mano_fit_store_verts(const ManoModel& m, const ManoLds& s, const ManoFitLds& f, float* verts, int b, int t) {
  if (!verts) return;
  for (int v = t; v < NV; v += 256) {
    float o[3];
    mano_skin_vertex(m, s, v, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) verts[((long)b * NV + v) * 3 + r] = o[r] * 1000.0f + f.P[58 + r];
  }
}

// VT: with the vertex term.  Without it the kernel is the joint fit as it was: every statement of that path is the one it had, and so are its bits.
template <bool VT>
__global__ __launch_bounds__(256) void mano_fit_kernel(ManoFitArgs a) {
  __shared__ ManoLds s;
  __shared__ ManoGradLds g;
  __shared__ ManoFitLds f;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* vc = VT ? a.vtarget + (long)b * NC : nullptr;
  const float* vu = VT ? a.vweight + (long)b * NV : nullptr;
  mano_fit_load(a.io, a.c.joint_map, f, nullptr, b, t);
  if (t < 61) f.M1[t] = f.M2[t] = 0.0f;
  float vstat[2];  // sum of the vertex weights, non-finite vertex targets under a positive weight
  if constexpr (VT) {
    float in[2];
    mano_vert_weights(vc, vu, t, in);
    mano_block_sum<2>(f, t, in, vstat);
  }
  mano_fit_status(f, VT ? vstat : nullptr, t);
  const bool ok = f.status == 0;  // otherwise: no init, no iteration, the state keeps its bits and the outputs evaluate it
  const int iters = ok ? a.c.iters : 0;
  mano_fit_eval<VT>(a.m, s, f, g.dv, t);
  if (iters > 0 && a.c.init_trans) mano_fit_init_trans<!VT>(f, vc, vu, g.dv, t);  // iters == 0 only evaluates
  if (t == 0) a.io.residual[(long)b * a.io.res_ld + 0] = mano_fit_residual(f);
  if constexpr (VT) {
    float in = mano_vert_distance(vc, vu, g.dv, &f.P[58], t), sum;
    mano_block_sum<1>(f, t, &in, &sum);
    if (t == 0) a.io.residual[(long)b * a.io.res_ld + 2] = f.sv > 0.0f ? sum / f.sv : 0.0f;
  } else {
    if (t == 0 && a.io.res_ld == 4) a.io.residual[(long)b * 4 + 2] = 0.0f;
  }
  const double b1 = (double)a.c.beta1, b2 = (double)a.c.beta2;
  const float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2);
  double b1k = 1.0, b2k = 1.0;
  for (int it = 1; it <= iters; ++it) {
    if (it > 1) mano_fit_eval<VT>(a.m, s, f, g.dv, t);
    // L = (1 / sum w) sum_i w_i |J_map[i] + t - y_i|^2 + lambda_shape |beta|^2 + lambda_pose |theta[3:]|^2, mm^2
    // (with the vertex term: + lambda_verts (1 / sum u) sum_v u_v |V_v + t - c_v|^2)
    if (t < 63) {
      const int i = t / 3, d = t - i * 3;
      f.gJ[i][d] = f.W[i] > 0.0f ? 2.0f * f.W[i] * (f.Jm[i][d] + f.P[58 + d] - f.Y[i][d]) / f.sw : 0.0f;
    }
    float vt[3] = {0.f, 0.f, 0.f};  // the vertex term's d L / d t
    if constexpr (VT) {
      float in[3];
      mano_vert_gradient(vc, vu, g.dv, &f.P[58], a.lambda_verts, f.sv, t, in);  // g.dv: the vertices of this state -> their gradient, in place
      mano_block_sum<3>(f, t, in, vt);
    } else {
      for (int c = t; c < NC; c += 256) g.dv[c] = 0.0f;
    }
    __syncthreads();
    if (t < 63) {  // x1000 output scale and the scatter to chain joints and tip vertices (kManoOut is a permutation: every slot is written once)
      const int i = t / 3, d = t - i * 3;
      const int src = kManoOut[i];
      const float v = f.gJ[i][d] * 1000.0f;
      if (src < NJ) g.dtg[src][d] = v;
      else if constexpr (VT) g.dv[kManoTip[src - NJ] * 3 + d] += v;  // a tip vertex: its own term, then its joint row's (one thread per slot)
      else g.dv[kManoTip[src - NJ] * 3 + d] = v;
    }
    if (t >= 64 && t < 67) {
      float sum = 0.f;
      for (int i = 0; i < 21; ++i) sum += f.gJ[i][t - 64];
      if constexpr (VT) sum += t == 64 ? vt[0] : (t == 65 ? vt[1] : vt[2]);
      f.Gd[58 + (t - 64)] = sum;
    }
    __syncthreads();
    mano_backward_lds(a.m, s, g, t);
    if (t < NJ) {
      float aa[3] = {f.P[t * 3 + 0], f.P[t * 3 + 1], f.P[t * 3 + 2]}, daa[3];
      if (t > 0)
        for (int i = 0; i < 3; ++i) aa[i] = a.m.hands_mean[(t - 1) * 3 + i] + aa[i];
      rodrigues_bwd(aa, g.dRj[t], daa);
      for (int i = 0; i < 3; ++i) f.Gd[t * 3 + i] = t > 0 ? fmaf(2.0f * a.c.lambda_pose, f.P[t * 3 + i], daa[i]) : daa[i];
    }
    if (t >= 64 && t < 74) f.Gd[48 + (t - 64)] = fmaf(2.0f * a.c.lambda_shape, f.P[48 + (t - 64)], g.dbeta[t - 64]);
    __syncthreads();
    // torch.optim.Adam (no weight decay, no amsgrad): the bias corrections in double, as the host-side optimiser has them
    b1k *= b1;
    b2k *= b2;
    if (t < 61) {
      const float lr = t < 48 ? a.c.lr_pose : (t < 58 ? a.c.lr_shape : a.c.lr_trans);
      const float step = (float)((double)lr / (1.0 - b1k)), bc2s = (float)sqrt(1.0 - b2k);
      const float gr = f.Gd[t];
      const float m1 = fmaf(omb1, gr - f.M1[t], f.M1[t]);
      const float m2 = fmaf(omb2 * gr, gr, f.M2[t] * a.c.beta2);
      f.M1[t] = m1;
      f.M2[t] = m2;
      f.P[t] = f.P[t] - step * (m1 / (sqrtf(m2) / bc2s + a.c.eps));
    }
    __syncthreads();
  }
  if (iters > 0) mano_fit_eval<VT>(a.m, s, f, g.dv, t);
  if (t == 0) {
    a.io.residual[(long)b * a.io.res_ld + 1] = mano_fit_residual(f);
    a.io.status[b] = f.status;
  }
  if constexpr (VT) {
    float in = mano_vert_distance(vc, vu, g.dv, &f.P[58], t), sum;
    mano_block_sum<1>(f, t, &in, &sum);
    if (t == 0) a.io.residual[(long)b * a.io.res_ld + 3] = f.sv > 0.0f ? sum / f.sv : 0.0f;
  } else {
    if (t == 0 && a.io.res_ld == 4) a.io.residual[(long)b * 4 + 3] = 0.0f;
  }
  mano_fit_store(a.io, a.c.joint_map, f, ok, b, t);
  mano_fit_store_verts(a.m, s, f, a.io.verts, b, t);
}

// ---------------------------------------------------------------------------------------------------------------
// Gauss-Newton fit: the joint fit's objective, state, targets and outputs, minimised by damped Gauss-Newton steps.  Per iteration:
//   r_i = sqrt(w_i / sw) (J_map[i] + t - y_i), 63 rows in mm;  J = d r / d p, 63 x 61, forward-mode, one column per lane;
//   A = J^T J + Lambda + mu diag(J^T J) + nu I,  g = J^T r + Lambda p,  A delta = g by Cholesky in LDS,  p <- p - delta.
// Stages of an iteration: mano_fit_eval (the Adam fit's, shared), mano_gn_tangent (J and r), the normal matrix (1891 lower entries and g, each a sum over
// the 63 rows in ascending order, held in registers by the thread that formed it), the factorisation (square-root-free Cholesky, one barrier per column,
// the forward substitution rides along as row 61), the back substitution (wave 0, shuffles).  No atomics; every sum has a fixed order.
// ---------------------------------------------------------------------------------------------------------------
constexpr int GN_P = 61, GN_R = 63, GN_SLOTS = 8;  // 61 * 62 / 2 + 61 = 1952 entries of the system over 256 threads

struct ManoGnArgs {
  ManoFitIo io;               // target is never null here
  ManoModel m;
  kpf_mano_fit_gn_cfg c;
  float *history, *jacobian;  // [B][iters + 1], [B][63][61]; each may be null
  int hist_ld;                // io.res_ld 2 and hist_ld 1: the layouts above.  4 and 2 (the mesh entry without a vertex term): residual [B][4] and history
                              // [B][iters + 1][2], the vertex distances (columns 2, 3 and entry 1 of each pair) written as 0
};

struct ManoGnLds {
  float J[GN_R][GN_P];       // d r / d p: rows in the MODEL's joint order (row h * 3 + d), already scaled by sqrt(w_h / sw); a row under weight 0 is 0
  float A[GN_P + 1][GN_P];   // lower triangle: column k as elimination step k finds it (A[k][k] the pivot d_k), L = A D^-1/2; row 61: g, eliminated alike
  float R[GN_R];             // r
  float SQ[21];              // sqrt(w_h / sw), model order
  int inv[21];               // model joint h is target row inv[h]
  float dJrS[10][NJ][3];     // j_regressor . shapedirs[k]: d Jr / d beta_k, a constant of the hand model (computed once per launch)
  float tipT[5][12];         // the five tips' blended transforms sum_j w[tip][j] G2[j] at the current state
  float tipW[5][NJ];         // their skinning weights
  int fail;
};

__device__ __forceinline__ float gn_lambda(const kpf_mano_fit_gn_cfg& c, int j) {  // Lambda's diagonal
  return (j >= 3 && j < 48) ? c.lambda_pose : ((j >= 48 && j < 58) ? c.lambda_shape : 0.0f);
}

// d rodrigues(aa) / d aa[k]: the tangent of the formula above operation by operation, its +1e-8 included (at aa == 0 the axis n = aa / |aa + 1e-8| is 0
// and its tangent 1 / |aa + 1e-8|: the product with sin(h) is the finite 1/2 the limit has)
__device__ __forceinline__ void rodrigues_tangent(const float* aa, int k, float* dR) {
  const float ap[3] = {aa[0] + 1e-8f, aa[1] + 1e-8f, aa[2] + 1e-8f};
  const float ang = sqrtf(ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2]);
  const float dang = (k == 0 ? ap[0] : (k == 1 ? ap[1] : ap[2])) / ang;
  const float h = ang * 0.5f, sn = sinf(h), cs = cosf(h), dh = 0.5f * dang;
  float q[4], dq[4];
  q[0] = cs;
  dq[0] = -sn * dh;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float n = aa[i] / ang;
    const float dn = (i == k ? 1.0f : 0.0f) / ang - aa[i] * dang / (ang * ang);
    q[i + 1] = sn * n;
    dq[i + 1] = cs * dh * n + sn * dn;
  }
  const float nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float dnq = (q[0] * dq[0] + q[1] * dq[1] + q[2] * dq[2] + q[3] * dq[3]) / nq;
  const float w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
  const float dw = (dq[0] - w * dnq) / nq, dx = (dq[1] - x * dnq) / nq, dy = (dq[2] - y * dnq) / nq, dz = (dq[3] - z * dnq) / nq;
  dR[0] = 2.0f * (w * dw + x * dx - y * dy - z * dz);
  dR[1] = 2.0f * (x * dy + y * dx - w * dz - z * dw);
  dR[2] = 2.0f * (w * dy + y * dw + x * dz + z * dx);
  dR[3] = 2.0f * (w * dz + z * dw + x * dy + y * dx);
  dR[4] = 2.0f * (w * dw - x * dx + y * dy - z * dz);
  dR[5] = 2.0f * (y * dz + z * dy - w * dx - x * dw);
  dR[6] = 2.0f * (x * dz + z * dx - w * dy - y * dw);
  dR[7] = 2.0f * (w * dx + x * dw + y * dz + z * dy);
  dR[8] = 2.0f * (w * dw - x * dx - y * dy + z * dz);
}

// What column `col` is: a pose column turns joint `a` about axis component `k`, a shape column moves beta_k, a translation column moves t_k
struct ManoGnColumn {
  int a;        // the joint whose rotation moves, or -1
  int shape;    // the beta that moves, or -1
  float dR[9];  // d Rj[a]
};

// The tangent of posed vertex v (metres) along one column, given dT = sum_j w[v][j] d G2[j] (accumulated by the caller while it walks the chain) and
// T = sum_j w[v][j] G2[j]:  d o = dT [p; 1] + T[:, :3] d p,  p = v_posed[v], d p = posedirs rows of the joint that turns . dR  |  shapedirs[k][v]  |  0.
// A stage function of the vertex index: the five tips use it today, a vertex term would call it for any v.
__device__ __forceinline__ void mano_gn_vertex_tangent(const ManoModel& m, const ManoLds& s, int v, const ManoGnColumn& col, const float* dT, const float* T,
                                                       float* o) {
  float dp[3] = {0.f, 0.f, 0.f};
  if (col.a > 0) {  // pmap = Rj[1:] - I: the nine entries of joint a
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float* row = m.poseT + (long)((col.a - 1) * 9 + i) * NC + v * 3;
#pragma unroll
      for (int d = 0; d < 3; ++d) dp[d] = fmaf(row[d], col.dR[i], dp[d]);
    }
  } else if (col.shape >= 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) dp[d] = m.shapeT[(long)col.shape * NC + v * 3 + d];
  }
  const float px = s.v[v * 3 + 0], py = s.v[v * 3 + 1], pz = s.v[v * 3 + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o[r] = (dT[r * 4 + 0] * px + dT[r * 4 + 1] * py + dT[r * 4 + 2] * pz + dT[r * 4 + 3]) +
           (T[r * 4 + 0] * dp[0] + T[r * 4 + 1] * dp[1] + T[r * 4 + 2] * dp[2]);
}

// What the vertex rows of the Gauss-Newton mesh fit keep in LDS beside the joint fit's state.  The system is padded to 64 columns:
// 0..60 the unknowns, 61 the residual r (so that g = J^T r falls out of the same product as J^T J), 62 zero, 63 spare (see dG2).
constexpr int GN_C = 64, GN_VB = 4, GN_CV = 4 * GN_VB, GN_CR = 3 * GN_CV, GN_CLD = 80, GN_DPLD = GN_CR + 1;
constexpr int GN_CHUNKS = (NV + GN_CV - 1) / GN_CV;

struct ManoGnVertLds {
  float dG2[NJ * 12][GN_C];  // entry i of d G2[j] along column c at [j * 12 + i][c]: the column lanes write and read it without a bank conflict.  Column 63 holds
                             // G2[j] itself, so that the lane that sums the tangent transforms of columns 0..60 sums the vertex's own transform T_v in lane 63
  float dR[48][9];           // d Rj[c / 3] along pose column c
  float dp[GN_C][GN_DPLD];   // d (v_posed) along column c for the chunk's 16 vertices x 3 coordinates (pose columns 3..47, shape columns 48..57), metres
  float chunk[GN_C * GN_C];  // 48 rows of [J | r | 0 0] at a stride of 80 floats (rows k .. k + 3 of a tile column fall into 64 different banks); after the
                             // last chunk: the 64 x 64 product
  float vm[NC];              // the skinned vertices of this state, mm, without the translation
  float w[GN_CV][NJ];        // the chunk's skinning weights: one coalesced load per thread, then wave-uniform LDS reads
  float c[NC], u[NV];        // the vertex targets (selected to 0 where the weight is not > 0) and weights, loaded once per launch: a row's scale and its
                             // residual then cost no global-memory latency inside the chunk loop
};

__device__ __forceinline__ void mano_gn_keep_rotation(ManoGnVertLds* x, int c, const float* dR) {
  if (c < 48)
#pragma unroll
    for (int i = 0; i < 9; ++i) x->dR[c][i] = dR[i];
}

__device__ __forceinline__ void mano_gn_keep_transform(ManoGnVertLds* x, int c, int j, const float* d2) {
#pragma unroll
  for (int i = 0; i < 12; ++i) x->dG2[j * 12 + i][c] = d2[i];
}

__device__ __forceinline__ void mano_gn_keep_spare(ManoGnVertLds* x, const ManoLds& s, int c) {  // lanes 61..63
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 12; ++i) x->dG2[j * 12 + i][c] = c == GN_C - 1 ? s.G2[j][i] : 0.0f;
}

// J and r of the state in s / f (after mano_fit_eval).  Lanes 0..60 of wave 0 each build one column forward-mode: the tangent transform is carried down
// the chain (a joint's parent is the root or the joint before it, so the root's and the previous joint's tangents in registers are enough) and the five
// tips' blended tangent transforms are accumulated on the way.  gout: null, or [63][61] for the unweighted columns in target-row order.
// All 256 threads; ends with a barrier.
// VT (the fit with the vertex term): every column lane also leaves what the vertex rows need in x -- its joint's rotation tangent and, joint by joint as it
// walks the chain, its tangent transforms d G2[j]; lanes 61..63 fill the three spare columns (zeros, and G2 itself in column 63).
template <bool VT>
__device__ __forceinline__ void mano_gn_tangent(const ManoModel& m, const ManoLds& s, const ManoFitLds& f, ManoGnLds& n, int t, float* gout,
                                                ManoGnVertLds* x = nullptr) {
  if (t >= 64 && t < 64 + 60) {  // the tips' blended transforms of this state, j ascending as mano_skin_transform
    const int k = (t - 64) / 12, i = (t - 64) % 12;
    float sum = 0.f;
    for (int j = 0; j < NJ; ++j) sum = fmaf(n.tipW[k][j], s.G2[j][i], sum);
    n.tipT[k][i] = sum;
  }
  if (t >= 128 && t < 128 + GN_R) {
    const int h = (t - 128) / 3, d = (t - 128) % 3;
    n.R[t - 128] = f.W[h] > 0.0f ? n.SQ[h] * (f.Jm[h][d] + f.P[58 + d] - f.Y[h][d]) : 0.0f;
  }
  __syncthreads();
  if (t < GN_P) {
    ManoGnColumn col;
    col.a = t < 48 ? t / 3 : -1;
    col.shape = (t >= 48 && t < 58) ? t - 48 : -1;
    const int td = t >= 58 ? t - 58 : -1;
#pragma unroll
    for (int i = 0; i < 9; ++i) col.dR[i] = 0.f;
    if (col.a >= 0) {
      float aa[3] = {f.P[col.a * 3 + 0], f.P[col.a * 3 + 1], f.P[col.a * 3 + 2]};
      if (col.a > 0)
        for (int i = 0; i < 3; ++i) aa[i] = m.hands_mean[(col.a - 1) * 3 + i] + aa[i];
      rodrigues_tangent(aa, t - col.a * 3, col.dR);
    }
    if constexpr (VT) mano_gn_keep_rotation(x, t, col.dR);
    auto put = [&](int h, int r, float metres) {  // model joint h, coordinate r: the column's entry in mm
      const float v = metres * 1000.0f + (r == td ? 1.0f : 0.0f);
      n.J[h * 3 + r][t] = f.W[h] > 0.0f ? n.SQ[h] * v : 0.0f;
      if (gout) gout[(n.inv[h] * 3 + r) * GN_P + t] = v;
    };
    float dG0[12], dGq[12], dG[12], acc[5][12];  // the root's, the previous joint's and this joint's tangent transform; the tips' blended ones
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int i = 0; i < 12; ++i) acc[k][i] = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) dG0[i] = dGq[i] = 0.f;
    for (int j = 0; j < NJ; ++j) {
      const int p = kManoParent[j];
      float dJ[3] = {0.f, 0.f, 0.f}, drel[3] = {0.f, 0.f, 0.f};
      if (col.shape >= 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          dJ[r] = n.dJrS[col.shape][j][r];
          drel[r] = p < 0 ? dJ[r] : dJ[r] - n.dJrS[col.shape][p][r];
        }
      }
      const bool turns = j == col.a;
      if (p < 0) {  // G[0] = [Rj[0] | Jr[0]]
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dG[r * 4 + c] = turns ? col.dR[r * 3 + c] : 0.f;
          dG[r * 4 + 3] = drel[r];
        }
      } else {  // G[j] = G[p] loc, loc = [Rj[j] | Jr[j] - Jr[p]]:  d G[j] = d G[p] loc + G[p] d loc
        float rel[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) rel[r] = s.Jr[j][r] - s.Jr[p][r];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float e0 = p == 0 ? dG0[r * 4 + 0] : dGq[r * 4 + 0], e1 = p == 0 ? dG0[r * 4 + 1] : dGq[r * 4 + 1];
          const float e2 = p == 0 ? dG0[r * 4 + 2] : dGq[r * 4 + 2], e3 = p == 0 ? dG0[r * 4 + 3] : dGq[r * 4 + 3];
          const float g0 = s.G[p][r * 4 + 0], g1 = s.G[p][r * 4 + 1], g2 = s.G[p][r * 4 + 2];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float sum = e0 * s.Rj[j][0 * 3 + c] + e1 * s.Rj[j][1 * 3 + c] + e2 * s.Rj[j][2 * 3 + c];
            if (turns) sum += g0 * col.dR[0 * 3 + c] + g1 * col.dR[1 * 3 + c] + g2 * col.dR[2 * 3 + c];
            dG[r * 4 + c] = sum;
          }
          dG[r * 4 + 3] = (e0 * rel[0] + e1 * rel[1] + e2 * rel[2] + e3) + (g0 * drel[0] + g1 * drel[1] + g2 * drel[2]);
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) put(j, r, dG[r * 4 + 3]);  // chain joint j is joints3d row j (kManoOut[i] == i for i < 16)
      // G2[j] = [Rg | tg - Rg Jr[j]]
      float d2[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        d2[r * 4 + 0] = dG[r * 4 + 0];
        d2[r * 4 + 1] = dG[r * 4 + 1];
        d2[r * 4 + 2] = dG[r * 4 + 2];
        d2[r * 4 + 3] = dG[r * 4 + 3] - (dG[r * 4 + 0] * s.Jr[j][0] + dG[r * 4 + 1] * s.Jr[j][1] + dG[r * 4 + 2] * s.Jr[j][2]) -
                        (s.G[j][r * 4 + 0] * dJ[0] + s.G[j][r * 4 + 1] * dJ[1] + s.G[j][r * 4 + 2] * dJ[2]);
      }
      if constexpr (VT) mano_gn_keep_transform(x, t, j, d2);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float w = n.tipW[k][j];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[k][i] = fmaf(w, d2[i], acc[k][i]);
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        if (j == 0) dG0[i] = dG[i];
        dGq[i] = dG[i];
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float o[3];
      mano_gn_vertex_tangent(m, s, kManoTip[k], col, acc[k], n.tipT[k], o);
#pragma unroll
      for (int r = 0; r < 3; ++r) put(kManoTipRow[k], r, o[r]);
    }
  } else if constexpr (VT) {
    if (t < 64) mano_gn_keep_spare(x, s, t);
  }
  __syncthreads();
}

// This thread's entries of the 62 x 61 system (rows 0..60: the lower triangle of A; row 61: g), the same for every iteration: i | j << 8, or -1.
// Rows a and 60 - a of the triangle hold 62 entries together: 31 pairs (row 30 pairs with itself), then the 61 entries of g.
__device__ __forceinline__ void mano_gn_slots(int t, int (&slot)[GN_SLOTS]) {
#pragma unroll
  for (int q = 0; q < GN_SLOTS; ++q) {
    const int e = t + 256 * q, pr = e / 62, k = e - pr * 62;
    int i = -1, j = 0;
    if (e >= 31 * 62) {
      if (e < 31 * 62 + GN_P) {
        i = GN_P;
        j = e - 31 * 62;
      }
    } else if (!(pr == 30 && k >= 31)) {
      j = k < GN_P - pr ? pr : 60 - pr;                          // the column (the smaller index)
      i = k < GN_P - pr ? pr + k : 60 - pr + (k - (GN_P - pr));  // the row (>= j)
    }
    slot[q] = i < 0 ? -1 : (i | (j << 8));
  }
}

// The system in val (each thread's entries, column 0 already in n.A) -> p <- p - delta.  False, and the state untouched, if a pivot is not > 0 or not finite.
// All 256 threads; begins with a barrier, and the caller ends the iteration with one.
__device__ __forceinline__ bool mano_gn_solve(ManoGnLds& n, ManoFitLds& f, const int (&slot)[GN_SLOTS], float (&val)[GN_SLOTS], int t) {
  __syncthreads();
  // Cholesky in its square-root-free form, right-looking, one barrier per column: A = C D^-1 C^T with C's column k the column as elimination step k
  // finds it (its head is the pivot d_k), so that L = C D^-1/2.  Step k subtracts c_ik c_jk / d_k from every entry right of column k; an entry is
  // written to LDS once, when the step before its column has made it final.  Row 61 takes part like any other: it ends as C D^-1/2 z, z = L^-1 g.
  for (int k = 0; k < GN_P; ++k) {
    const float dk = n.A[k][k];
    if (t == 0 && !(dk > 0.0f && isfinite(dk))) n.fail = 1;
#pragma unroll
    for (int q = 0; q < GN_SLOTS; ++q) {
      const int i = slot[q] & 255, j = slot[q] >> 8;
      if (j > k) {  // an empty slot has j < 0
        val[q] = fmaf(-n.A[i][k], n.A[j][k] / dk, val[q]);
        if (j == k + 1) n.A[i][j] = val[q];
      }
    }
    __syncthreads();
  }
  if (n.fail) return false;
  if ((t >> 6) == 0) {  // back substitution C^T delta = (row 61): lane i holds row 61's entry i and d_i, delta_k travels by a shuffle
    float z = t < GN_P ? n.A[GN_P][t] : 0.0f, delta = 0.0f;
    const float d = t < GN_P ? n.A[t][t] : 1.0f;
    for (int k = GN_P - 1; k >= 0; --k) {
      const float dk = __shfl(z, k, 64) / __shfl(d, k, 64);
      if (t == k) delta = dk;
      if (t < k) z = fmaf(-n.A[k][t], dk, z);
    }
    if (t < GN_P) f.P[t] = f.P[t] - delta;
  }
  return true;
}

// The constants of a launch of either Gauss-Newton kernel, in two parts.  Before mano_fit_status, whose barriers publish them: the tips' skinning weights
// (threads 128..207) and fail (thread 255).
__device__ __forceinline__ void mano_gn_setup_tips(const ManoModel& m, ManoGnLds& n, int t) {
  if (t >= 128 && t < 128 + 5 * NJ) n.tipW[(t - 128) / NJ][(t - 128) % NJ] = m.skin[(long)kManoTip[(t - 128) / NJ] * NJ + (t - 128) % NJ];
  if (t == 255) n.fail = 0;
}

// After mano_fit_status (ok = the fit runs): sqrt(w_h / sw) (threads 0..20) and, if a tangent will be formed, d Jr / d beta = j_regressor . shapedirs: 48 dot
// products of length 778 per beta, a wave per beta.  No barrier of its own: both are first read in mano_gn_tangent, and the mano_fit_eval every caller runs
// before that ends with one -- a caller that reads SQ or dJrS sooner must add its own.
__device__ __forceinline__ void mano_gn_setup(const ManoModel& m, const ManoFitLds& f, ManoGnLds& n, bool ok, bool tangent, int t) {
  const int wave = t >> 6, lane = t & 63;
  if (t < 21) n.SQ[t] = (ok && f.W[t] > 0.0f) ? sqrtf(f.W[t] / f.sw) : 0.0f;
  if (!tangent) return;
  for (int k = wave; k < 10; k += 4) {
    float acc[NJ * 3];
#pragma unroll
    for (int o = 0; o < NJ * 3; ++o) acc[o] = 0.f;
    for (int v = lane; v < NV; v += 64) {
      const float sx = m.shapeT[(long)k * NC + v * 3 + 0], sy = m.shapeT[(long)k * NC + v * 3 + 1], sz = m.shapeT[(long)k * NC + v * 3 + 2];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float w = m.jreg[(long)j * NV + v];
        acc[j * 3 + 0] = fmaf(w, sx, acc[j * 3 + 0]);
        acc[j * 3 + 1] = fmaf(w, sy, acc[j * 3 + 1]);
        acc[j * 3 + 2] = fmaf(w, sz, acc[j * 3 + 2]);
      }
    }
#pragma unroll
    for (int o = 0; o < NJ * 3; ++o) {
      const float sum = wave_sum(acc[o]);
      if (lane == 0) n.dJrS[k][o / 3][o % 3] = sum;
    }
  }
}

// History entry `it` (one thread): the mean weighted joint distance and, where the history is [iters + 1][2], the vertex distance beside it
__device__ __forceinline__ void mano_gn_hist_put(float* hist, int hist_ld, int it, float res, float dv) {
  hist[it * hist_ld] = res;
  if (hist_ld == 2) hist[it * 2 + 1] = dv;
}

// After the last iteration (one thread): once the fit has stopped (`from`: the first entry the loop has not written, or the one a failed iteration left)
// the state no longer moves, and the remaining entries repeat the last one
__device__ __forceinline__ void mano_gn_hist_tail(float* hist, int hist_ld, int from, int last, float res, float dv) {
  if (!hist) return;
  for (int it = from; it <= last; ++it) mano_gn_hist_put(hist, hist_ld, it, res, dv);
}

__global__ __launch_bounds__(256) void mano_fit_gn_kernel(ManoGnArgs a) {
  __shared__ ManoLds s;
  __shared__ ManoFitLds f;
  __shared__ ManoGnLds n;
  const int b = blockIdx.x, t = threadIdx.x;
  mano_fit_load(a.io, a.c.joint_map, f, n.inv, b, t);
  mano_gn_setup_tips(a.m, n, t);
  mano_fit_status(f, nullptr, t);
  const bool ok = f.status == 0;  // otherwise: no init, no iteration, the state keeps its bits and the outputs evaluate it
  const int iters = ok ? a.c.iters : 0;
  float* hist = a.history ? a.history + (long)b * (a.c.iters + 1) * a.hist_ld : nullptr;
  float* jac = a.jacobian ? a.jacobian + (long)b * GN_R * GN_P : nullptr;
  mano_gn_setup(a.m, f, n, ok, iters > 0 || jac, t);
  mano_fit_eval<false>(a.m, s, f, nullptr, t);
  if (iters > 0 && a.c.init_trans) mano_fit_init_trans<false>(f, nullptr, nullptr, nullptr, t);
  if (t == 0) a.io.residual[(long)b * a.io.res_ld + 0] = mano_fit_residual(f);
  if (iters == 0 && jac) mano_gn_tangent<false>(a.m, s, f, n, t, jac);  // only evaluates: the entry Jacobian is still reported
  int slot[GN_SLOTS];
  mano_gn_slots(t, slot);
  int done = 0, st4 = 0;
  for (int it = 1; it <= iters; ++it) {
    if (it > 1) mano_fit_eval<false>(a.m, s, f, nullptr, t);
    if (t == 0 && hist) mano_gn_hist_put(hist, a.hist_ld, it - 1, mano_fit_residual(f), 0.0f);
    mano_gn_tangent<false>(a.m, s, f, n, t, it == 1 ? jac : nullptr);
    // the normal matrix's lower triangle with the damped diagonal, and g as row 61: every thread forms its entries, each a sum over the 63 rows in
    // ascending order, and keeps them in registers through the factorisation
    float val[GN_SLOTS];
#pragma unroll
    for (int q = 0; q < GN_SLOTS; ++q) {
      const int i = slot[q] & 255, j = slot[q] >> 8;
      val[q] = 0.f;
      if (slot[q] < 0) continue;
      float sum = 0.f;
      if (i == GN_P) {
        for (int r = 0; r < GN_R; ++r) sum = fmaf(n.J[r][j], n.R[r], sum);
        sum = fmaf(gn_lambda(a.c, j), f.P[j], sum);
      } else {
        for (int r = 0; r < GN_R; ++r) sum = fmaf(n.J[r][j], n.J[r][i], sum);
        if (i == j) sum = fmaf(a.c.mu, sum, sum + gn_lambda(a.c, j)) + a.c.nu;
      }
      val[q] = sum;
      if (j == 0) n.A[i][0] = sum;
    }
    if (!mano_gn_solve(n, f, slot, val, t)) {  // a pivot that is not > 0 or not finite: stop, the state holds the last completed iteration
      st4 = 4;
      break;
    }
    done = it;
    __syncthreads();
  }
  if (done > 0) mano_fit_eval<false>(a.m, s, f, nullptr, t);
  if (t == 0) {
    const float res = mano_fit_residual(f);
    a.io.residual[(long)b * a.io.res_ld + 1] = res;
    a.io.status[b] = f.status | st4;
    mano_gn_hist_tail(hist, a.hist_ld, st4 ? done : iters, a.c.iters, res, 0.0f);
    if (a.io.res_ld == 4) a.io.residual[(long)b * 4 + 2] = a.io.residual[(long)b * 4 + 3] = 0.0f;
  }
  mano_fit_store(a.io, a.c.joint_map, f, ok, b, t);
  mano_fit_store_verts(a.m, s, f, a.io.verts, b, t);
}

// ---------------------------------------------------------------------------------------------------------------
// Gauss-Newton mesh fit: the iteration above with 2334 more rows, sqrt(lambda_verts u_v / sv) (V_v + t - c_v).  Per iteration, after
// mano_fit_eval<true> (all 778 vertices) and mano_gn_tangent<true> (J and r of the joints; every column's d G2[j] left in LDS):
//   the vertex rows in 49 chunks of 16 vertices -- a wave takes four vertices, a lane one of the 64 columns, and sums dT = sum_j w[v][j] d G2[j] for its
//   four vertices from one read of d G2[j] (lane 63 sums T_v itself that way); d v_posed of the chunk is formed once by all 256 threads from coalesced
//   reads of posedirs / shapedirs; row = scale (dT [p; 1] + T[:, :3] d p) in mm, column 61 = scale (V + t - c);
//   the product [J | r]^T [J | r] on v_mfma_f32_16x16x4_f32: wave w holds tile row w (4 tiles of 16 x 16) in registers across the joint rows and all chunks,
//   k ascending, so N = J^T J is its leading 61 x 61 block and g = J^T r its row 61;
//   the spill to LDS, Lambda and the damping, and the joint fit's factorisation and back substitution (mano_gn_solve).
// ---------------------------------------------------------------------------------------------------------------
struct ManoMeshGnArgs {
  ManoFitIo io;                    // target may be null (no joint carries weight); res_ld is 4
  const float *vtarget, *vweight;  // never null here
  ManoModel m;
  kpf_mano_fit_gn_cfg c;
  float lambda_verts;
  float *history, *jacobian, *vjacobian;  // [B][iters + 1][2], [B][63][61], [B][2334][61]; each may be null
};

// Chunk ch's 48 rows into x.chunk (vjac: null, or the unweighted rows of every vertex, [2334][61]).  All 256 threads; ends with a barrier, and its inner
// barrier also separates the previous chunk's product from this chunk's rows.
// PLANE: a vertex contributes one row, its three contracted with the normal n_v (nrm: this sample's [778][3] in global memory, 48 components per chunk);
// the other two of its rows are zeros, so that the chunk, the product and the two-level sum keep their shape and order.  vjac stays unprojected.
template <bool PLANE>
__device__ __forceinline__ void mano_gn_vertex_chunk(const ManoModel& m, const ManoLds& s, const ManoFitLds& f, ManoGnVertLds& x, float lambda, int ch, int t,
                                                     float* vjac, const float* nrm = nullptr) {
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, base = ch * GN_CV;
  int vq[GN_VB];  // this wave's vertices; past the last one: the last one's loads, and zero rows
#pragma unroll
  for (int q = 0; q < GN_VB; ++q) vq[q] = min(base + wave * GN_VB + q, NV - 1);
  x.w[t >> 4][t & 15] = m.skin[(long)min(base + (t >> 4), NV - 1) * NJ + (t & 15)];
#pragma unroll
  for (int e = t; e < 15 * GN_CR; e += 256) {  // pmap = Rj[1:] - I: joint a's nine rows of posedirs serve its three columns
    const int a = e / GN_CR + 1, vd = e % GN_CR, c = base * 3 + vd;
    float p[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = c < NC ? m.poseT[(long)((a - 1) * 9 + i) * NC + c] : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 9; ++i) sum = fmaf(p[i], x.dR[a * 3 + k][i], sum);
      x.dp[a * 3 + k][vd] = sum;
    }
  }
#pragma unroll
  for (int e = t; e < 10 * GN_CR; e += 256) {
    const int k = e / GN_CR, vd = e % GN_CR, c = base * 3 + vd;
    x.dp[48 + k][vd] = c < NC ? m.shapeT[(long)k * NC + c] : 0.f;
  }
  __syncthreads();
  float dT[GN_VB][12];
#pragma unroll
  for (int q = 0; q < GN_VB; ++q)
#pragma unroll
    for (int i = 0; i < 12; ++i) dT[q][i] = 0.f;
#pragma unroll 4
  for (int j = 0; j < NJ; ++j) {
    float d[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) d[i] = x.dG2[j * 12 + i][lane];
#pragma unroll
    for (int q = 0; q < GN_VB; ++q) {
      const float w = x.w[wave * GN_VB + q][j];
#pragma unroll
      for (int i = 0; i < 12; ++i) dT[q][i] = fmaf(w, d[i], dT[q][i]);
    }
  }
  const bool moves = lane >= 3 && lane < 58;  // v_posed does not move with the root's rotation or the translation
#pragma unroll
  for (int q = 0; q < GN_VB; ++q) {
    const int v = vq[q], row0 = (wave * GN_VB + q) * 3;
    const bool valid = base + wave * GN_VB + q < NV;
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dT[q][i]), GN_C - 1));
    const float u = x.u[v];
    const bool on = valid && u > 0.0f;  // a row under weight 0 is selected out, never multiplied
    const float scale = on ? sqrtf(lambda * u / f.sv) : 0.0f;
    const float px = s.v[v * 3 + 0], py = s.v[v * 3 + 1], pz = s.v[v * 3 + 2];
    const float d0 = moves ? x.dp[lane][row0 + 0] : 0.f, d1 = moves ? x.dp[lane][row0 + 1] : 0.f, d2 = moves ? x.dp[lane][row0 + 2] : 0.f;
    float pl = 0.f;  // PLANE: n_v . (this lane's three entries)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float o = (dT[q][r * 4 + 0] * px + dT[q][r * 4 + 1] * py + dT[q][r * 4 + 2] * pz + dT[q][r * 4 + 3]) +
                      (T[r * 4 + 0] * d0 + T[r * 4 + 1] * d1 + T[r * 4 + 2] * d2);
      const float val = o * 1000.0f + (lane - 58 == r ? 1.0f : 0.0f);
      if (vjac && valid && lane < GN_P) vjac[(long)(v * 3 + r) * GN_P + lane] = val;
      if constexpr (PLANE) {
        float e = 0.f;
        if (on && lane < GN_P) e = val;
        else if (on && lane == GN_P) e = x.vm[v * 3 + r] + f.P[58 + r] - x.c[v * 3 + r];
        pl = fmaf(on ? nrm[v * 3 + r] : 0.0f, e, pl);  // a normal under weight 0 is selected out, never multiplied
        if (r > 0) x.chunk[(row0 + r) * GN_CLD + lane] = 0.0f;
      } else {
        float e = 0.f;
        if (on && lane < GN_P) e = scale * val;
        else if (on && lane == GN_P) e = scale * (x.vm[v * 3 + r] + f.P[58 + r] - x.c[v * 3 + r]);
        x.chunk[(row0 + r) * GN_CLD + lane] = e;
      }
    }
    if constexpr (PLANE) x.chunk[row0 * GN_CLD + lane] = on ? scale * pl : 0.0f;
  }
  __syncthreads();
}

// mano_vert_distance along the normal: sum u_v |n_v . (V_v + t - c_v)|
__device__ __forceinline__ float mano_vert_plane_distance(const float* c, const float* u, const float* vm, const float* nrm, const float* tr, int t) {
  float sum = 0.f;
  for (int v = t; v < NV; v += 256) {
    const float w = u[v];
    if (!(w > 0.0f)) continue;
    const float r0 = vm[v * 3 + 0] + tr[0] - c[v * 3 + 0], r1 = vm[v * 3 + 1] + tr[1] - c[v * 3 + 1], r2 = vm[v * 3 + 2] + tr[2] - c[v * 3 + 2];
    sum = fmaf(w, fabsf(nrm[v * 3 + 0] * r0 + nrm[v * 3 + 1] * r1 + nrm[v * 3 + 2] * r2), sum);
  }
  return sum;
}

template <bool PLANE>
__device__ __forceinline__ float mano_mesh_gn_vert_distance(ManoFitLds& f, const ManoGnVertLds& x, const float* nrm, int t) {
  float in, sum;
  if constexpr (PLANE) in = mano_vert_plane_distance(x.c, x.u, x.vm, nrm, &f.P[58], t);
  else in = mano_vert_distance(x.c, x.u, x.vm, &f.P[58], t);
  mano_block_sum<1>(f, t, &in, &sum);
  return f.sv > 0.0f ? sum / f.sv : 0.0f;
}

// PLANE: the vertex term is point-to-plane (one row per vertex, see mano_gn_vertex_chunk).  Without it the kernel is the mesh fit as it was, statement by
// statement.  vnormal [B][778][3], fixed for the launch, is an argument of its own so that the arguments of the instantiation without it stay what they were.
template <bool PLANE>
__global__ __launch_bounds__(256) void mano_fit_mesh_gn_kernel(ManoMeshGnArgs a, const float* vnormal) {
  __shared__ ManoLds s;
  __shared__ ManoFitLds f;
  __shared__ ManoGnLds n;
  __shared__ ManoGnVertLds x;
  const int b = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const float* vc = a.vtarget + (long)b * NC;
  const float* vu = a.vweight + (long)b * NV;
  const float* vn = PLANE ? vnormal + (long)b * NC : nullptr;
  mano_fit_load(a.io, a.c.joint_map, f, n.inv, b, t);
  mano_gn_setup_tips(a.m, n, t);
  for (int v = t; v < NV; v += 256) {
    const float u = vu[v];
    x.u[v] = u;
#pragma unroll
    for (int d = 0; d < 3; ++d) x.c[v * 3 + d] = u > 0.0f ? vc[v * 3 + d] : 0.0f;  // a target of weight 0 is selected out, not multiplied
  }
  float vstat[2];  // sum of the vertex weights, non-finite vertex targets under a positive weight
  {
    float in[2];
    mano_vert_weights(vc, vu, t, in);
    if constexpr (PLANE) {  // a normal under a positive weight that is not finite counts as such a target does
      for (int v = t; v < NV; v += 256)
        if (vu[v] > 0.0f && !(isfinite(vn[v * 3 + 0]) && isfinite(vn[v * 3 + 1]) && isfinite(vn[v * 3 + 2]))) in[1] += 1.0f;
    }
    mano_block_sum<2>(f, t, in, vstat);
  }
  mano_fit_status(f, vstat, t);
  const bool ok = f.status == 0;  // otherwise: no init, no iteration, the state keeps its bits and the outputs evaluate it
  const int iters = ok ? a.c.iters : 0;
  float* hist = a.history ? a.history + (long)b * (a.c.iters + 1) * 2 : nullptr;
  float* jac = a.jacobian ? a.jacobian + (long)b * GN_R * GN_P : nullptr;
  float* vjac = a.vjacobian ? a.vjacobian + (long)b * NC * GN_P : nullptr;
  mano_gn_setup(a.m, f, n, ok, iters > 0 || jac || vjac, t);
  mano_fit_eval<true>(a.m, s, f, x.vm, t);
  if (iters > 0 && a.c.init_trans) mano_fit_init_trans<false>(f, x.c, x.u, x.vm, t);
  {
    const float dv = mano_mesh_gn_vert_distance<PLANE>(f, x, vn, t);
    if (t == 0) {
      a.io.residual[(long)b * 4 + 0] = mano_fit_residual(f);
      a.io.residual[(long)b * 4 + 2] = dv;
    }
  }
  if (iters == 0 && (jac || vjac)) {  // only evaluates: the entry Jacobians are still reported
    mano_gn_tangent<true>(a.m, s, f, n, t, jac, &x);
    if (vjac)
      for (int ch = 0; ch < GN_CHUNKS; ++ch) mano_gn_vertex_chunk<PLANE>(a.m, s, f, x, a.lambda_verts, ch, t, vjac, vn);
  }
  int slot[GN_SLOTS];
  mano_gn_slots(t, slot);
  int done = 0, st4 = 0;
  for (int it = 1; it <= iters; ++it) {
    if (it > 1) mano_fit_eval<true>(a.m, s, f, x.vm, t);
    if (hist) {
      const float dv = mano_mesh_gn_vert_distance<PLANE>(f, x, vn, t);
      if (t == 0) mano_gn_hist_put(hist, 2, it - 1, mano_fit_residual(f), dv);
    }
    mano_gn_tangent<true>(a.m, s, f, n, t, it == 1 ? jac : nullptr, &x);
    // wave w's tile row of [J | r]^T [J | r]: lane l feeds element [k0 + l / 16][tile * 16 + l % 16] of the rows to both operands and holds
    // rows w * 16 + 4 (l / 16) + 0..3 of column tile * 16 + l % 16 in acc[tile].  The sum has two levels, both in a fixed order: the joint rows and each
    // chunk's 48 rows are summed from zero (part) and the 50 partial sums are added in turn -- one chain over all 2397 rows would round about five
    // times as much, and that error of J^T J was the largest term of the state's distance from the float64 iteration
    f32x4 acc[4], part[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[tj] = part[tj] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < 64; k0 += 4) {  // the 63 joint rows, as mano_gn_tangent left them (a row under weight 0 is 0)
      const int k = k0 + (lane >> 4);
      auto el = [&](int c) { return k < GN_R ? (c < GN_P ? n.J[k][c] : (c == GN_P ? n.R[k] : 0.0f)) : 0.0f; };
      const float av = el(wave * 16 + (lane & 15));
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) part[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, el(tj * 16 + (lane & 15)), part[tj], 0, 0, 0);
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[tj] = part[tj];
    for (int ch = 0; ch < GN_CHUNKS; ++ch) {
      mano_gn_vertex_chunk<PLANE>(a.m, s, f, x, a.lambda_verts, ch, t, it == 1 ? vjac : nullptr, vn);
      const float* rows = x.chunk + (lane >> 4) * GN_CLD + (lane & 15);
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) part[tj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < GN_CR; k0 += 4) {
        const float av = rows[k0 * GN_CLD + wave * 16];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) part[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, rows[k0 * GN_CLD + tj * 16], part[tj], 0, 0, 0);
      }
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) acc[tj] += part[tj];
    }
    __syncthreads();  // the last chunk's rows have been read: x.chunk becomes the 64 x 64 product
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) x.chunk[(wave * 16 + 4 * (lane >> 4) + r) * GN_C + tj * 16 + (lane & 15)] = acc[tj][r];
    __syncthreads();
    float val[GN_SLOTS];  // the lower triangle with Lambda and the damping, and g as row 61: the joint fit's layout
#pragma unroll
    for (int q = 0; q < GN_SLOTS; ++q) {
      const int i = slot[q] & 255, j = slot[q] >> 8;
      val[q] = 0.f;
      if (slot[q] < 0) continue;
      float sum = x.chunk[i * GN_C + j];
      if (i == GN_P) sum = fmaf(gn_lambda(a.c, j), f.P[j], sum);
      else if (i == j) sum = fmaf(a.c.mu, sum, sum + gn_lambda(a.c, j)) + a.c.nu;
      val[q] = sum;
      if (j == 0) n.A[i][0] = sum;
    }
    if (!mano_gn_solve(n, f, slot, val, t)) {  // a pivot that is not > 0 or not finite: stop, the state holds the last completed iteration
      st4 = 4;
      break;
    }
    done = it;
    __syncthreads();
  }
  if (done > 0) mano_fit_eval<true>(a.m, s, f, x.vm, t);
  {
    const float dv = mano_mesh_gn_vert_distance<PLANE>(f, x, vn, t);
    if (t == 0) {
      const float res = mano_fit_residual(f);
      a.io.residual[(long)b * 4 + 1] = res;
      a.io.residual[(long)b * 4 + 3] = dv;
      a.io.status[b] = f.status | st4;
      mano_gn_hist_tail(hist, 2, st4 ? done : iters, a.c.iters, res, dv);
    }
  }
  mano_fit_store(a.io, a.c.joint_map, f, ok, b, t);
  if (a.io.verts)  // the skinned vertices are in LDS: a plain sum, where the other two kernels' re-skinning contracts o * 1000 + t
    for (int c = t; c < NC; c += 256) a.io.verts[(long)b * NC + c] = x.vm[c] + f.P[58 + c % 3];
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// The fit entries' host side.  `name` prefixes every refusal.
// ---------------------------------------------------------------------------------------------------------------
struct ManoFitHost {
  ManoModel m;
  ManoFitIo io;
};

static ManoFitHost mano_fit_host(const float* target, const float* weight, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                                 const float* j_regressor, const float* skin_weights, const float* hands_mean, float* pose_aa, float* betas, float* trans,
                                 float* verts, float* joints, float* rotmat, float* residual, int res_ld, int* status) {
  return ManoFitHost{ManoModel{shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean},
                     ManoFitIo{target, weight, pose_aa, betas, trans, verts, joints, rotmat, residual, status, res_ld}};
}

// The thirteen pointers no fit entry does without (target, weight, verts and rotmat may be null)
static int mano_check_fit_pointers(const char* name, const ManoFitHost& h, const void* cfg) {
  KPF_REQUIRE(h.m.shapeT && h.m.poseT && h.m.vtmpl && h.m.jreg && h.m.skin && h.m.hands_mean && cfg && h.io.pose && h.io.betas && h.io.trans && h.io.joints &&
                  h.io.residual && h.io.status,
              "%s: null pointer", name);
  return KPF_OK;
}

// Those pointers, then B (the mesh Gauss-Newton entries check their argument combinations in between)
static int mano_check_fit_common(const char* name, const ManoFitHost& h, const void* cfg, int B) {
  if (const int rc = mano_check_fit_pointers(name, h, cfg)) return rc;
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  return KPF_OK;
}

static int mano_check_joint_map(const char* name, const int* map) {
  unsigned seen = 0;
  for (int i = 0; i < 21; ++i) {
    KPF_REQUIRE(map[i] >= 0 && map[i] < 21, "%s: joint_map[%d]=%d outside [0, 21)", name, i, map[i]);
    seen |= 1u << map[i];
  }
  KPF_REQUIRE(seen == (1u << 21) - 1, "%s: joint_map is not a permutation", name);
  return KPF_OK;
}

// The two Adam entries: vert_target / vert_weight select the instantiation with the vertex term
static int mano_fit_launch(const char* name, const ManoFitHost& h, const float* vert_target, const float* vert_weight, const kpf_mano_fit_cfg* cfg,
                           float lambda_verts, int B, void* stream) {
  if (const int rc = mano_check_fit_common(name, h, cfg, B)) return rc;
  KPF_REQUIRE(cfg->iters >= 0 && cfg->iters <= 1000, "%s: iters=%d outside [0, 1000]", name, cfg->iters);
  KPF_REQUIRE(cfg->beta1 >= 0.f && cfg->beta1 < 1.f && cfg->beta2 >= 0.f && cfg->beta2 < 1.f && cfg->eps >= 0.f,
              "%s: bad Adam constants beta1=%g beta2=%g eps=%g", name, cfg->beta1, cfg->beta2, cfg->eps);
  if (const int rc = mano_check_joint_map(name, cfg->joint_map)) return rc;
  const ManoFitArgs a{h.io, vert_target, vert_weight, h.m, *cfg, lambda_verts};
  if (vert_target && vert_weight) hipLaunchKernelGGL(mano_fit_kernel<true>, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(mano_fit_kernel<false>, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

extern "C" int kpf_mano_fit_f32(const float* target, const float* weight, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                                const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_cfg* cfg,
                                float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                                int B, void* stream) {
  KPF_REQUIRE(target, "kpf_mano_fit_f32: null pointer");
  return mano_fit_launch("kpf_mano_fit_f32", mano_fit_host(target, weight, shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean, pose_aa,
                                                           betas, trans, verts, joints, rotmat, residual, 2, status),
                         nullptr, nullptr, cfg, 0.0f, B, stream);
}

extern "C" int kpf_mano_fit_mesh_f32(const float* target, const float* weight, const float* vert_target, const float* vert_weight,
                                     const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
                                     const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_cfg* cfg, float* pose_aa, float* betas,
                                     float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status, int B, void* stream) {
  KPF_REQUIRE(cfg, "kpf_mano_fit_mesh_f32: null pointer");
  KPF_REQUIRE((vert_target == nullptr) == (vert_weight == nullptr), "kpf_mano_fit_mesh_f32: vert_target and vert_weight go together");
  KPF_REQUIRE(cfg->lambda_verts >= 0.f, "kpf_mano_fit_mesh_f32: lambda_verts=%g is negative", cfg->lambda_verts);
  kpf_mano_fit_cfg c;
  c.iters = cfg->iters;
  c.lr_pose = cfg->lr_pose; c.lr_shape = cfg->lr_shape; c.lr_trans = cfg->lr_trans;
  c.beta1 = cfg->beta1; c.beta2 = cfg->beta2; c.eps = cfg->eps;
  c.lambda_shape = cfg->lambda_shape; c.lambda_pose = cfg->lambda_pose;
  c.init_trans = cfg->init_trans;
  for (int i = 0; i < 21; ++i) c.joint_map[i] = cfg->joint_map[i];
  return mano_fit_launch("kpf_mano_fit_mesh_f32", mano_fit_host(target, weight, shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean,
                                                                pose_aa, betas, trans, verts, joints, rotmat, residual, 4, status),
                         vert_target, vert_weight, &c, cfg->lambda_verts, B, stream);
}

// The iteration count and damping of the three Gauss-Newton entries (the mesh entries' cfg: converted first)
static int mano_check_gn_cfg(const char* name, const kpf_mano_fit_gn_cfg& c) {
  KPF_REQUIRE(c.iters >= 0 && c.iters <= 64, "%s: iters=%d outside [0, 64]", name, c.iters);
  KPF_REQUIRE(c.mu >= 0.f && c.nu >= 0.f && isfinite(c.mu) && isfinite(c.nu), "%s: bad damping mu=%g nu=%g", name, c.mu, c.nu);
  return KPF_OK;
}

// The joint Gauss-Newton kernel: res_ld 2 and hist_ld 1 for its own entry, 4 and 2 for a mesh entry without a vertex term
static int mano_gn_launch(const char* name, const ManoFitHost& h, const kpf_mano_fit_gn_cfg& c, float* history, float* jacobian, int hist_ld, int B,
                          void* stream) {
  const ManoGnArgs a{h.io, h.m, c, history, jacobian, hist_ld};
  hipLaunchKernelGGL(mano_fit_gn_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

extern "C" int kpf_mano_fit_gn_f32(const float* target, const float* weight, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                                   const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_gn_cfg* cfg,
                                   float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                                   float* history, float* jacobian, int B, void* stream) {
  const char* name = "kpf_mano_fit_gn_f32";
  KPF_REQUIRE(target, "%s: null pointer", name);
  const ManoFitHost h = mano_fit_host(target, weight, shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean, pose_aa, betas, trans, verts,
                                      joints, rotmat, residual, 2, status);
  if (const int rc = mano_check_fit_common(name, h, cfg, B)) return rc;
  if (const int rc = mano_check_gn_cfg(name, *cfg)) return rc;
  if (const int rc = mano_check_joint_map(name, cfg->joint_map)) return rc;
  return mano_gn_launch(name, h, *cfg, history, jacobian, 1, B, stream);
}

// The two Gauss-Newton mesh entries: `name` prefixes every refusal; vert_normal selects the instantiation with the point-to-plane vertex term
static int mano_mesh_gn_launch(const char* name, const float* target, const float* weight, const float* vert_target, const float* vert_weight,
                               const float* vert_normal, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                               const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_gn_cfg* cfg,
                               float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                               float* history, float* jacobian, float* vert_jacobian, int B, void* stream) {
  const ManoFitHost h = mano_fit_host(target, weight, shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean, pose_aa, betas, trans, verts,
                                      joints, rotmat, residual, 4, status);
  if (const int rc = mano_check_fit_pointers(name, h, cfg)) return rc;
  KPF_REQUIRE((vert_target == nullptr) == (vert_weight == nullptr), "%s: vert_target and vert_weight go together", name);
  KPF_REQUIRE(target || vert_target, "%s: neither joint nor vertex targets", name);
  KPF_REQUIRE(vert_target || !vert_jacobian, "%s: vert_jacobian needs the vertex term", name);
  KPF_REQUIRE(vert_target || !vert_normal, "%s: vert_normal needs the vertex term", name);
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  kpf_mano_fit_gn_cfg c;
  c.iters = cfg->iters;
  c.mu = cfg->mu; c.nu = cfg->nu;
  c.lambda_shape = cfg->lambda_shape; c.lambda_pose = cfg->lambda_pose;
  c.init_trans = cfg->init_trans;
  for (int i = 0; i < 21; ++i) c.joint_map[i] = cfg->joint_map[i];
  if (const int rc = mano_check_gn_cfg(name, c)) return rc;
  KPF_REQUIRE(cfg->lambda_verts >= 0.f && isfinite(cfg->lambda_verts), "%s: lambda_verts=%g is negative or not finite", name, cfg->lambda_verts);
  if (const int rc = mano_check_joint_map(name, c.joint_map)) return rc;
  if (!vert_target) return mano_gn_launch(name, h, c, history, jacobian, 2, B, stream);  // no vertex term: the joint fit's kernel, its bits
  const ManoMeshGnArgs a{h.io, vert_target, vert_weight, h.m, c, cfg->lambda_verts, history, jacobian, vert_jacobian};
  if (vert_normal) hipLaunchKernelGGL(mano_fit_mesh_gn_kernel<true>, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, vert_normal);
  else hipLaunchKernelGGL(mano_fit_mesh_gn_kernel<false>, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, vert_normal);
  return kpf_check_launch(name);
}

extern "C" int kpf_mano_fit_mesh_gn_f32(const float* target, const float* weight, const float* vert_target, const float* vert_weight,
                                        const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor,
                                        const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_gn_cfg* cfg, float* pose_aa,
                                        float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                                        float* history, float* jacobian, float* vert_jacobian, int B, void* stream) {
  return mano_mesh_gn_launch("kpf_mano_fit_mesh_gn_f32", target, weight, vert_target, vert_weight, nullptr, shapedirs_t, posedirs_t, v_template, j_regressor,
                             skin_weights, hands_mean, cfg, pose_aa, betas, trans, verts, joints, rotmat, residual, status, history, jacobian, vert_jacobian,
                             B, stream);
}

extern "C" int kpf_mano_fit_mesh_gn_plane_f32(const float* target, const float* weight, const float* vert_target, const float* vert_weight,
                                              const float* vert_normal, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                                              const float* j_regressor, const float* skin_weights, const float* hands_mean,
                                              const kpf_mano_fit_mesh_gn_cfg* cfg, float* pose_aa, float* betas, float* trans, float* verts, float* joints,
                                              float* rotmat, float* residual, int* status, float* history, float* jacobian, float* vert_jacobian, int B,
                                              void* stream) {
  return mano_mesh_gn_launch("kpf_mano_fit_mesh_gn_plane_f32", target, weight, vert_target, vert_weight, vert_normal, shapedirs_t, posedirs_t, v_template,
                             j_regressor, skin_weights, hands_mean, cfg, pose_aa, betas, trans, verts, joints, rotmat, residual, status, history, jacobian,
                             vert_jacobian, B, stream);
}
