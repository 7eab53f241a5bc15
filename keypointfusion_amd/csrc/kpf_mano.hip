// The MANO hand model (model/mano_head.py:144-225, util/manopth/manopth/manolayer.py:106-273) as three kernels, one 256-thread workgroup per sample:
//   kpf_mano_forward_f32   6D rotations + betas -> vertices, joints, rotations, axis-angle            (eval path of heads.ManoHeadPlan)
//   kpf_mano_backward_f32  its derivative: recomputes the forward in LDS, then walks the stages backwards (heads_train.ManoLayerHip)
//   kpf_mano_fit_f32       Adam on pose / shape / translation against 21 target joints, every iteration inside the one launch (mano_fit.ManoFitter)
//   kpf_mano_fit_mesh_f32  the same fit with a vertex term (778 weighted vertex targets): the second instantiation of the fit kernel
//   kpf_mano_fit_gn_f32    the joint fit by damped Gauss-Newton: forward-mode Jacobian, normal matrix and Cholesky solve in LDS (its own kernel, further down)
//   kpf_mano_fit_mesh_gn_f32  the Gauss-Newton fit with the vertex term: 2334 more rows, J^T J on the fp32 MFMA (its own kernel, after the joint fit's)
//   kpf_mano_assoc_f32     depth points -> nearest vertex, per-vertex centroid and weight: the vertex targets of the fit above (its own kernel, further down)
//   kpf_mano_normals_f32   area-weighted vertex normals of the fitted mesh from the model's faces (its own kernel, after the association's)
//   kpf_mano_assoc_vis_f32 the association over the vertices that face the camera, with the point-to-plane distance among its stats
//   kpf_mano_fit_mesh_gn_plane_f32  the Gauss-Newton mesh fit with one point-to-plane row per vertex: the second instantiation of that kernel
// The fits share the stage functions below; the forward's arithmetic is the text it had in kpf_aux.hip (tests/test_heads_gpu.py pins its bits).
// Every reduction has a fixed order (wave butterflies, then a fixed sum over the four waves) and there are no atomics: a replay is bit-identical and a
// sample's bits do not depend on B or on its position in the batch.
#include <math.h>

#include "kpf_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// MANO: 6D rotations -> rotation matrices -> axis-angle -> (Rodrigues again, as the reference does) -> blend shapes, joint
// regression, kinematic chain, linear-blend skinning.  One 256-thread workgroup per sample; the sample's 778 x 3 vertices live
// in LDS from the shape blend to the final skinning.  Blend-shape bases are read transposed ([k][778*3]) so lanes coalesce.
// ---------------------------------------------------------------------------------------------------------------
constexpr int NV = 778, NJ = 16, NC = NV * 3;
__constant__ int kManoParent[16] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14};
// joints3d[i] = jtr21[ORDER[OBMAN2MANO[i]]] with jtr21 = [16 chain joints, 5 finger-tip vertices]
// (manolayer.py:251-261 then model/mano_head.py:7-16,221)
__constant__ int kManoOut[21] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17, 18, 20, 19, 16};
__constant__ int kManoTip[5] = {745, 317, 444, 556, 673};
__constant__ int kManoTipRow[5] = {20, 16, 17, 19, 18};  // the joints3d row that holds tip k: kManoOut[kManoTipRow[k]] == 16 + k

__device__ void rot6d_to_mat(const float* x, float* R) {  // model/mano_head.py:144-153 (b1,b2,b3 are columns)
  float a1[3] = {x[0], x[1], x[2]}, a2[3] = {x[3], x[4], x[5]};
  float n1 = fmaxf(sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12f);
  float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
  const float d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
  float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
  float n2 = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
  float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
  float b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
  for (int r = 0; r < 3; ++r) {
    R[r * 3 + 0] = b1[r];
    R[r * 3 + 1] = b2[r];
    R[r * 3 + 2] = b3[r];
  }
}

// d (F.normalize(v)) -> d v, with v's norm n (before the clamp) and b = v / max(n, 1e-12): where the clamp is active the divisor is a constant
__device__ __forceinline__ void normalize_bwd(const float* b, float n, const float* db, float* dv) {
  if (n > 1e-12f) {
    const float p = b[0] * db[0] + b[1] * db[1] + b[2] * db[2];
    for (int i = 0; i < 3; ++i) dv[i] = (db[i] - b[i] * p) / n;
  } else {
    for (int i = 0; i < 3; ++i) dv[i] = db[i] / 1e-12f;
  }
}

__device__ void rot6d_to_mat_bwd(const float* x, const float* dR, float* dx) {
  float a1[3] = {x[0], x[1], x[2]}, a2[3] = {x[3], x[4], x[5]};
  const float m1 = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), n1 = fmaxf(m1, 1e-12f);
  float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
  const float d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
  float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
  const float m2 = sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), n2 = fmaxf(m2, 1e-12f);
  float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
  float db1[3], db2[3], db3[3];
  for (int r = 0; r < 3; ++r) {
    db1[r] = dR[r * 3 + 0];
    db2[r] = dR[r * 3 + 1];
    db3[r] = dR[r * 3 + 2];
  }
  // b3 = b1 x b2:  d b1 += b2 x d b3,  d b2 += d b3 x b1
  db1[0] += b2[1] * db3[2] - b2[2] * db3[1];
  db1[1] += b2[2] * db3[0] - b2[0] * db3[2];
  db1[2] += b2[0] * db3[1] - b2[1] * db3[0];
  db2[0] += db3[1] * b1[2] - db3[2] * b1[1];
  db2[1] += db3[2] * b1[0] - db3[0] * b1[2];
  db2[2] += db3[0] * b1[1] - db3[1] * b1[0];
  float du[3], da1[3];
  normalize_bwd(b2, m2, db2, du);
  const float dd = -(du[0] * b1[0] + du[1] * b1[1] + du[2] * b1[2]);  // u = a2 - d b1
  for (int i = 0; i < 3; ++i) db1[i] += -d * du[i] + dd * a2[i];      // d = b1 . a2
  normalize_bwd(b1, m1, db1, da1);
  for (int i = 0; i < 3; ++i) {
    dx[i] = da1[i];
    dx[3 + i] = du[i] + dd * b1[i];
  }
}

// model/mano_head.py:84-141 on the transpose: the un-normalised quaternion of the branch the matrix selects, and the branch's trace term t.
// Branch b -> q = (A0, t, S2, S1) | (A1, S2, t, S0) | (A2, S1, S0, t) | (t, A0, A1, A2) with A the antisymmetric and S the symmetric pairs.
__device__ __forceinline__ int mat_to_quat_raw(const float* R, float* q, float& t) {
  // t = R^T: t[i][j] = R[j][i]
#define T_(i, j) R[(j) * 3 + (i)]
  const float m00 = T_(0, 0), m11 = T_(1, 1), m22 = T_(2, 2);
  int branch;
  if (m22 < 1e-6f) {
    if (m00 > m11) {
      t = 1 + m00 - m11 - m22;
      q[0] = T_(1, 2) - T_(2, 1); q[1] = t; q[2] = T_(0, 1) + T_(1, 0); q[3] = T_(2, 0) + T_(0, 2);
      branch = 0;
    } else {
      t = 1 - m00 + m11 - m22;
      q[0] = T_(2, 0) - T_(0, 2); q[1] = T_(0, 1) + T_(1, 0); q[2] = t; q[3] = T_(1, 2) + T_(2, 1);
      branch = 1;
    }
  } else {
    if (m00 < -m11) {
      t = 1 - m00 - m11 + m22;
      q[0] = T_(0, 1) - T_(1, 0); q[1] = T_(2, 0) + T_(0, 2); q[2] = T_(1, 2) + T_(2, 1); q[3] = t;
      branch = 2;
    } else {
      t = 1 + m00 + m11 + m22;
      q[0] = t; q[1] = T_(1, 2) - T_(2, 1); q[2] = T_(2, 0) - T_(0, 2); q[3] = T_(0, 1) - T_(1, 0);
      branch = 3;
    }
  }
#undef T_
  return branch;
}

__device__ void mat_to_aa(const float* R, float* aa) {  // model/mano_head.py:84-141 (on the transpose), :49-81, :171-173
  float q[4], t;
  mat_to_quat_raw(R, q, t);
  const float inv = 0.5f / sqrtf(t);
  for (int i = 0; i < 4; ++i) q[i] *= inv;
  const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float s = sqrtf(s2), c = q[0];
  const float two_theta = 2.0f * (c < 0.0f ? atan2f(-s, -c) : atan2f(s, c));
  const float k = s2 > 0.0f ? two_theta / s : 2.0f;
  for (int i = 0; i < 3; ++i) {
    const float v = q[i + 1] * k;
    aa[i] = isnan(v) ? 0.0f : v;
  }
}

// d aa -> d R.  Autograd's conventions: no gradient through a component the isnan select replaced.  At s2 == 0 (identity) the forward takes k = 2 and
// this returns that branch's derivative (d q_i = 2 d aa_i), where autograd of the reference formula has sqrt'(0) under its `where` and gives NaN.
__device__ void mat_to_aa_bwd(const float* R, const float* daa, float* dR) {
  float qr[4], t;
  const int branch = mat_to_quat_raw(R, qr, t);
  const float inv = 0.5f / sqrtf(t);
  float q[4];
  for (int i = 0; i < 4; ++i) q[i] = qr[i] * inv;
  const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float s = sqrtf(s2), c = q[0];
  const float two_theta = 2.0f * (c < 0.0f ? atan2f(-s, -c) : atan2f(s, c));
  const float k = s2 > 0.0f ? two_theta / s : 2.0f;
  float dq[4] = {0.f, 0.f, 0.f, 0.f}, dk = 0.f;
  for (int i = 0; i < 3; ++i) {
    const float g = isnan(q[i + 1] * k) ? 0.0f : daa[i];
    dq[i + 1] = g * k;
    dk = fmaf(g, q[i + 1], dk);
  }
  if (s2 > 0.0f) {
    const float dtt = dk / s;                         // k = two_theta / s
    float ds = -dk * two_theta / s2;
    const float h2 = s2 + c * c;                      // both atan2 forms: d theta / d s = c / (s^2 + c^2), d theta / d c = -s / (s^2 + c^2)
    ds = fmaf(2.0f * dtt, c / h2, ds);
    dq[0] = -2.0f * dtt * s / h2;
    const float ds2 = ds / (2.0f * s);                // s = sqrt(s2)
    for (int i = 1; i < 4; ++i) dq[i] = fmaf(2.0f * ds2, q[i], dq[i]);
  }
  // q = qr * inv, inv = 0.5 t^-1/2
  float dinv = 0.f, dqr[4];
  for (int i = 0; i < 4; ++i) {
    dqr[i] = dq[i] * inv;
    dinv = fmaf(dq[i], qr[i], dinv);
  }
  const float tslot[4] = {dqr[1], dqr[2], dqr[3], dqr[0]};
  float dA[3], dS[3] = {0.f, 0.f, 0.f};
  float dt = -dinv * inv / (2.0f * t);
  float s00, s11, s22;
  if (branch == 0) {
    dt += tslot[0]; dA[0] = dqr[0]; dA[1] = 0.f; dA[2] = 0.f; dS[2] = dqr[2]; dS[1] = dqr[3];
    s00 = 1.f; s11 = -1.f; s22 = -1.f;
  } else if (branch == 1) {
    dt += tslot[1]; dA[0] = 0.f; dA[1] = dqr[0]; dA[2] = 0.f; dS[2] = dqr[1]; dS[0] = dqr[3];
    s00 = -1.f; s11 = 1.f; s22 = -1.f;
  } else if (branch == 2) {
    dt += tslot[2]; dA[0] = 0.f; dA[1] = 0.f; dA[2] = dqr[0]; dS[1] = dqr[1]; dS[0] = dqr[2];
    s00 = -1.f; s11 = -1.f; s22 = 1.f;
  } else {
    dt += tslot[3]; dA[0] = dqr[1]; dA[1] = dqr[2]; dA[2] = dqr[3];
    s00 = 1.f; s11 = 1.f; s22 = 1.f;
  }
  // A0 = T12 - T21, A1 = T20 - T02, A2 = T01 - T10; S0 = T12 + T21, S1 = T20 + T02, S2 = T01 + T10; d R[j][i] = d T[i][j]
#define DT_(i, j) dR[(j) * 3 + (i)]
  DT_(0, 0) = s00 * dt; DT_(1, 1) = s11 * dt; DT_(2, 2) = s22 * dt;
  DT_(1, 2) = dS[0] + dA[0]; DT_(2, 1) = dS[0] - dA[0];
  DT_(2, 0) = dS[1] + dA[1]; DT_(0, 2) = dS[1] - dA[1];
  DT_(0, 1) = dS[2] + dA[2]; DT_(1, 0) = dS[2] - dA[2];
#undef DT_
}

__device__ void rodrigues(const float* aa, float* R) {  // util/manopth/manopth/rodrigues_layer.py:16-57
  const float ax = aa[0] + 1e-8f, ay = aa[1] + 1e-8f, az = aa[2] + 1e-8f;
  const float ang = sqrtf(ax * ax + ay * ay + az * az);
  const float h = ang * 0.5f, sn = sinf(h), cs = cosf(h);
  float q[4] = {cs, sn * (aa[0] / ang), sn * (aa[1] / ang), sn * (aa[2] / ang)};
  const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
  R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;     R[2] = 2 * wy + 2 * xz;
  R[3] = 2 * wz + 2 * xy;   R[4] = w2 - x2 + y2 - z2;   R[5] = 2 * yz - 2 * wx;
  R[6] = 2 * xz - 2 * wy;   R[7] = 2 * wx + 2 * yz;     R[8] = w2 - x2 - y2 + z2;
}

__device__ void rodrigues_bwd(const float* aa, const float* g, float* daa) {  // g = d R (9) -> d aa (3), operation by operation as autograd does
  const float ap[3] = {aa[0] + 1e-8f, aa[1] + 1e-8f, aa[2] + 1e-8f};
  const float ang = sqrtf(ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2]);
  const float h = ang * 0.5f, sn = sinf(h), cs = cosf(h);
  const float nv[3] = {aa[0] / ang, aa[1] / ang, aa[2] / ang};
  const float q[4] = {cs, sn * nv[0], sn * nv[1], sn * nv[2]};
  const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  const float dqh[4] = {2.0f * (w * (g[0] + g[4] + g[8]) + z * (g[3] - g[1]) + y * (g[2] - g[6]) + x * (g[7] - g[5])),
                        2.0f * (x * (g[0] - g[4] - g[8]) + y * (g[1] + g[3]) + z * (g[2] + g[6]) + w * (g[7] - g[5])),
                        2.0f * (y * (g[4] - g[0] - g[8]) + x * (g[1] + g[3]) + w * (g[2] - g[6]) + z * (g[5] + g[7])),
                        2.0f * (z * (g[8] - g[0] - g[4]) + w * (g[3] - g[1]) + x * (g[2] + g[6]) + y * (g[5] + g[7]))};
  const float p = w * dqh[0] + x * dqh[1] + y * dqh[2] + z * dqh[3];
  const float dq[4] = {(dqh[0] - w * p) / n, (dqh[1] - x * p) / n, (dqh[2] - y * p) / n, (dqh[3] - z * p) / n};
  const float dh = -sn * dq[0] + cs * (nv[0] * dq[1] + nv[1] * dq[2] + nv[2] * dq[3]);
  const float dn[3] = {sn * dq[1], sn * dq[2], sn * dq[3]};
  const float dang = 0.5f * dh - (dn[0] * aa[0] + dn[1] * aa[1] + dn[2] * aa[2]) / (ang * ang);
  for (int i = 0; i < 3; ++i) daa[i] = dn[i] / ang + dang * (ap[i] / ang);
}

struct ManoModel {
  const float *shapeT, *poseT, *vtmpl, *jreg, *skin, *hands_mean;  // [10][NC], [135][NC], [NC], [16][778], [778][16], [45]
};

struct ManoLds {                  // one sample's forward state
  float v[NC];                    // v_shaped -> v_posed (-> posed vertices in the forward kernel), metres
  float Rj[NJ][9];                // rotations the MANO layer uses (Rodrigues of the axis-angle pose)
  float pmap[135];
  float beta[10];
  float Jr[NJ][3];
  float G[NJ][12], G2[NJ][12];    // global joint transforms (3x4), and with the rest pose removed
};

// Joint t's rotation from its axis-angle (hands_mean already added) and its rows of the pose map
__device__ __forceinline__ void mano_set_rotation(ManoLds& s, int t, const float* aa) {
  rodrigues(aa, s.Rj[t]);
  if (t > 0)
    for (int i = 0; i < 9; ++i) s.pmap[(t - 1) * 9 + i] = s.Rj[t][i] - ((i == 0 || i == 4 || i == 8) ? 1.0f : 0.0f);
}

// beta, Rj and pmap written by the caller -> v = v_posed, Jr, G, G2.  All 256 threads; barriers at entry and exit.
__device__ __forceinline__ void mano_blend_chain(const ManoModel& a, ManoLds& s, int t) {
  __syncthreads();
  for (int c = t; c < NC; c += 256) {  // shape blend
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) v = fmaf(a.shapeT[(long)k * NC + c], s.beta[k], v);
    s.v[c] = v + a.vtmpl[c];
  }
  __syncthreads();
  {  // joint regression from the shaped (un-posed) vertices: 48 dot products of length 778, 12 per wave
    const int wave = t >> 6, lane = t & 63;
    for (int o = wave; o < NJ * 3; o += 4) {
      const int j = o / 3, d = o - j * 3;
      float sum = 0.f;
      for (int v = lane; v < NV; v += 64) sum = fmaf(a.jreg[(long)j * NV + v], s.v[v * 3 + d], sum);
      sum = wave_sum(sum);
      if (lane == 0) s.Jr[j][d] = sum;
    }
  }
  __syncthreads();
  for (int c = t; c < NC; c += 256) {  // pose blend (in place: each coordinate is touched by exactly one thread)
    float v = 0.f;
    for (int k = 0; k < 135; ++k) v = fmaf(a.poseT[(long)k * NC + c], s.pmap[k], v);
    s.v[c] += v;
  }
  if (t == 0) {  // kinematic chain, parents precede children
    for (int j = 0; j < NJ; ++j) {
      const int p = kManoParent[j];
      float loc[12];
      for (int r = 0; r < 3; ++r) {
        loc[r * 4 + 0] = s.Rj[j][r * 3 + 0];
        loc[r * 4 + 1] = s.Rj[j][r * 3 + 1];
        loc[r * 4 + 2] = s.Rj[j][r * 3 + 2];
        loc[r * 4 + 3] = p < 0 ? s.Jr[j][r] : s.Jr[j][r] - s.Jr[p][r];
      }
      if (p < 0) {
        for (int i = 0; i < 12; ++i) s.G[j][i] = loc[i];
      } else {
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 4; ++c) {
            float sum = s.G[p][r * 4 + 0] * loc[0 * 4 + c] + s.G[p][r * 4 + 1] * loc[1 * 4 + c] + s.G[p][r * 4 + 2] * loc[2 * 4 + c];
            if (c == 3) sum += s.G[p][r * 4 + 3];
            s.G[j][r * 4 + c] = sum;
          }
      }
      for (int r = 0; r < 3; ++r) {
        const float corr = s.G[j][r * 4 + 0] * s.Jr[j][0] + s.G[j][r * 4 + 1] * s.Jr[j][1] + s.G[j][r * 4 + 2] * s.Jr[j][2];
        s.G2[j][r * 4 + 0] = s.G[j][r * 4 + 0];
        s.G2[j][r * 4 + 1] = s.G[j][r * 4 + 1];
        s.G2[j][r * 4 + 2] = s.G[j][r * 4 + 2];
        s.G2[j][r * 4 + 3] = s.G[j][r * 4 + 3] - corr;
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void mano_skin_transform(const ManoModel& a, const ManoLds& s, int v, float* T) {  // T = sum_j w[v][j] G2[j]
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = 0.f;
  for (int j = 0; j < NJ; ++j) {
    const float w = a.skin[(long)v * NJ + j];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = fmaf(w, s.G2[j][i], T[i]);
  }
}

__device__ __forceinline__ void mano_skin_vertex(const ManoModel& a, const ManoLds& s, int v, float* o) {  // linear-blend skinning of v_posed[v], metres
  float T[12];
  mano_skin_transform(a, s, v, T);
  const float px = s.v[v * 3 + 0], py = s.v[v * 3 + 1], pz = s.v[v * 3 + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = T[r * 4 + 0] * px + T[r * 4 + 1] * py + T[r * 4 + 2] * pz + T[r * 4 + 3];
}

struct ManoArgs {
  const float* pose6d;  // [B][ld6] (first 96 used)
  const float* betas;   // [B][ldb] (first 10 used)
  int ld6, ldb;
  ManoModel m;
  float *verts, *joints, *rotmat, *aa;  // [B][778][3], [B][21][3], [B][16][9], [B][48]
};

__global__ __launch_bounds__(256) void mano_kernel(ManoArgs a) {
  __shared__ ManoLds s;
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 10) s.beta[t] = a.betas[(long)b * a.ldb + t];
  if (t < NJ) {
    float R[9], aa[3];
    rot6d_to_mat(a.pose6d + (long)b * a.ld6 + t * 6, R);
    mat_to_aa(R, aa);
    for (int i = 0; i < 9; ++i) a.rotmat[((long)b * NJ + t) * 9 + i] = R[i];
    for (int i = 0; i < 3; ++i) a.aa[(long)b * 48 + t * 3 + i] = aa[i];
    if (t > 0)
      for (int i = 0; i < 3; ++i) aa[i] = a.m.hands_mean[(t - 1) * 3 + i] + aa[i];
    mano_set_rotation(s, t, aa);
  }
  mano_blend_chain(a.m, s, t);
  for (int v = t; v < NV; v += 256) {  // linear-blend skinning
    float o[3];
    mano_skin_vertex(a.m, s, v, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      s.v[v * 3 + r] = o[r];
      a.verts[((long)b * NV + v) * 3 + r] = o[r] * 1000.0f;
    }
  }
  __syncthreads();
  if (t < 21 * 3) {
    const int i = t / 3, d = t - i * 3;
    const int src = kManoOut[i];
    const float v = src < NJ ? s.G[src][d * 4 + 3] : s.v[kManoTip[src - NJ] * 3 + d];
    a.joints[((long)b * 21 + i) * 3 + d] = v * 1000.0f;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Backward of the stages between the rotations and the outputs (metres).  In: s after mano_blend_chain (v = v_posed), g.dv = d (posed vertex) for every
// vertex and g.dtg[j] = d (chain joint j's position), both written by the caller and followed by a barrier.  Out: g.dRj = d Rj, g.dbeta; ends with a barrier.
// Stages, in the order run: skinning, rest-pose removal, chain (children before parents), pose blend, joint regression, shape blend.
// ---------------------------------------------------------------------------------------------------------------
struct ManoGradLds {
  float dv[NC];            // d posed vertex -> d v_posed -> d v_shaped
  float part[4][NJ * 12];  // the four waves' partial sums of d G2
  float dG[NJ][12];        // d G2 -> [d (global rotation) | d (global translation)]
  float dtg[NJ][3];
  float dJr[NJ][3];
  float dRj[NJ][9];
  float dpmap[135];
  float dbeta[10];
};

__device__ __forceinline__ void mano_backward_lds(const ManoModel& a, const ManoLds& s, ManoGradLds& g, int t) {
  const int wave = t >> 6, lane = t & 63;
  // skinning: o_v = T_v [p_v; 1], T_v = sum_j w[v][j] G2[j]  ->  d G2[j] = sum_v w[v][j] [d o_v p_v^T | d o_v]: lanes over vertices, one butterfly per entry
  for (int j = 0; j < NJ; ++j) {
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;
    for (int v = t; v < NV; v += 256) {
      const float w = a.skin[(long)v * NJ + j];
      const float px = s.v[v * 3 + 0], py = s.v[v * 3 + 1], pz = s.v[v * 3 + 2];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float wd = w * g.dv[v * 3 + r];
        acc[r * 4 + 0] = fmaf(wd, px, acc[r * 4 + 0]);
        acc[r * 4 + 1] = fmaf(wd, py, acc[r * 4 + 1]);
        acc[r * 4 + 2] = fmaf(wd, pz, acc[r * 4 + 2]);
        acc[r * 4 + 3] += wd;
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const float sum = wave_sum(acc[i]);
      if (lane == 0) g.part[wave][j * 12 + i] = sum;
    }
  }
  for (int v = t; v < NV; v += 256) {  // d p_v = T_v[:, :3]^T d o_v, in place (this thread is the only one that touches vertex v)
    float T[12];
    mano_skin_transform(a, s, v, T);
    const float d0 = g.dv[v * 3 + 0], d1 = g.dv[v * 3 + 1], d2 = g.dv[v * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) g.dv[v * 3 + c] = T[0 * 4 + c] * d0 + T[1 * 4 + c] * d1 + T[2 * 4 + c] * d2;
  }
  __syncthreads();
  if (t < NJ * 12) g.dG[t / 12][t % 12] = ((g.part[0][t] + g.part[1][t]) + g.part[2][t]) + g.part[3][t];
  __syncthreads();
  if (t < NJ) {  // rest-pose removal: G2 = [Rg | tg - Rg Jr]
    const float e0 = g.dG[t][3], e1 = g.dG[t][7], e2 = g.dG[t][11];
    for (int c = 0; c < 3; ++c) {
      g.dJr[t][c] = -(s.G[t][0 * 4 + c] * e0 + s.G[t][1 * 4 + c] * e1 + s.G[t][2 * 4 + c] * e2);
      g.dG[t][0 * 4 + c] -= e0 * s.Jr[t][c];
      g.dG[t][1 * 4 + c] -= e1 * s.Jr[t][c];
      g.dG[t][2 * 4 + c] -= e2 * s.Jr[t][c];
    }
    for (int r = 0; r < 3; ++r) g.dG[t][r * 4 + 3] += g.dtg[t][r];
  }
  __syncthreads();
  if (t == 0) {  // kinematic chain, children before parents: Rg_j = Rg_p R_j, tg_j = Rg_p (Jr_j - Jr_p) + tg_p
    for (int j = NJ - 1; j > 0; --j) {
      const int p = kManoParent[j];
      float rel[3], dt[3];
      for (int r = 0; r < 3; ++r) {
        rel[r] = s.Jr[j][r] - s.Jr[p][r];
        dt[r] = g.dG[j][r * 4 + 3];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          g.dRj[j][r * 3 + c] = s.G[p][0 * 4 + r] * g.dG[j][0 * 4 + c] + s.G[p][1 * 4 + r] * g.dG[j][1 * 4 + c] + s.G[p][2 * 4 + r] * g.dG[j][2 * 4 + c];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          g.dG[p][r * 4 + c] += g.dG[j][r * 4 + 0] * s.Rj[j][c * 3 + 0] + g.dG[j][r * 4 + 1] * s.Rj[j][c * 3 + 1] + g.dG[j][r * 4 + 2] * s.Rj[j][c * 3 + 2] +
                                dt[r] * rel[c];
        g.dG[p][r * 4 + 3] += dt[r];
      }
      for (int c = 0; c < 3; ++c) {
        const float u = s.G[p][0 * 4 + c] * dt[0] + s.G[p][1 * 4 + c] * dt[1] + s.G[p][2 * 4 + c] * dt[2];
        g.dJr[j][c] += u;
        g.dJr[p][c] -= u;
      }
    }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) g.dRj[0][r * 3 + c] = g.dG[0][r * 4 + c];
      g.dJr[0][r] += g.dG[0][r * 4 + 3];
    }
  }
  for (int k = wave; k < 135; k += 4) {  // pose blend: d pmap[k] = posedirs[k] . d v_posed
    float sum = 0.f;
    for (int c = lane; c < NC; c += 64) sum = fmaf(a.poseT[(long)k * NC + c], g.dv[c], sum);
    sum = wave_sum(sum);
    if (lane == 0) g.dpmap[k] = sum;
  }
  __syncthreads();
  for (int v = t; v < NV; v += 256) {  // joint regression: d v_shaped = d v_posed + J_regressor^T d Jr
    float e[3] = {g.dv[v * 3 + 0], g.dv[v * 3 + 1], g.dv[v * 3 + 2]};
    for (int j = 0; j < NJ; ++j) {
      const float w = a.jreg[(long)j * NV + v];
#pragma unroll
      for (int d = 0; d < 3; ++d) e[d] = fmaf(w, g.dJr[j][d], e[d]);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) g.dv[v * 3 + d] = e[d];
  }
  if (t >= 64 && t < 64 + 135) g.dRj[1 + (t - 64) / 9][(t - 64) % 9] += g.dpmap[t - 64];  // pmap = Rj[1:] - I
  __syncthreads();
  for (int k = wave; k < 10; k += 4) {  // shape blend: d beta[k] = shapedirs[k] . d v_shaped
    float sum = 0.f;
    for (int c = lane; c < NC; c += 64) sum = fmaf(a.shapeT[(long)k * NC + c], g.dv[c], sum);
    sum = wave_sum(sum);
    if (lane == 0) g.dbeta[k] = sum;
  }
  __syncthreads();
}

struct ManoBwdArgs {
  const float *pose6d, *betas;
  int ld6, ldb;
  ManoModel m;
  const float *d_verts, *d_joints, *d_rotmat, *d_aa;  // each may be null
  float *d_pose6d, *d_betas;
  int ldd6, lddb;
};

__global__ __launch_bounds__(256) void mano_backward_kernel(ManoBwdArgs a) {
  __shared__ ManoLds s;
  __shared__ ManoGradLds g;
  const int b = blockIdx.x, t = threadIdx.x;
  float x6[6], R[9], aa[3];  // joint t's input, rotation and axis-angle (threads 0..15), kept for the last three stages
  if (t < 10) s.beta[t] = a.betas[(long)b * a.ldb + t];
  if (t < NJ) {
    for (int i = 0; i < 6; ++i) x6[i] = a.pose6d[(long)b * a.ld6 + t * 6 + i];
    rot6d_to_mat(x6, R);
    mat_to_aa(R, aa);
    if (t > 0)
      for (int i = 0; i < 3; ++i) aa[i] = a.m.hands_mean[(t - 1) * 3 + i] + aa[i];
    mano_set_rotation(s, t, aa);
  }
  // x1000 output scale and tip gather: a tip vertex also receives its joints3d row's gradient
  for (int c = t; c < NC; c += 256) g.dv[c] = a.d_verts ? a.d_verts[(long)b * NC + c] * 1000.0f : 0.0f;
  if (t < NJ * 3) g.dtg[t / 3][t % 3] = a.d_joints ? a.d_joints[(long)b * 63 + t] * 1000.0f : 0.0f;  // kManoOut[i] == i for i < 16
  __syncthreads();
  if (t < 15 && a.d_joints) g.dv[kManoTip[t / 3] * 3 + t % 3] += a.d_joints[(long)b * 63 + kManoTipRow[t / 3] * 3 + t % 3] * 1000.0f;
  mano_blend_chain(a.m, s, t);
  mano_backward_lds(a.m, s, g, t);
  if (t < NJ) {
    float daa[3], dR[9], dx[6];
    rodrigues_bwd(aa, g.dRj[t], daa);
    if (a.d_aa)
      for (int i = 0; i < 3; ++i) daa[i] += a.d_aa[(long)b * 48 + t * 3 + i];
    mat_to_aa_bwd(R, daa, dR);
    if (a.d_rotmat)
      for (int i = 0; i < 9; ++i) dR[i] += a.d_rotmat[((long)b * NJ + t) * 9 + i];
    rot6d_to_mat_bwd(x6, dR, dx);
    for (int i = 0; i < 6; ++i) a.d_pose6d[(long)b * a.ldd6 + t * 6 + i] = dx[i];
  }
  if (t >= 64 && t < 74) a.d_betas[(long)b * a.lddb + (t - 64)] = g.dbeta[t - 64];
}

// ---------------------------------------------------------------------------------------------------------------
// Fit: Adam on (pose_aa 48, betas 10, trans 3) of one sample against 21 target joints; every iteration inside the launch, state and moments in LDS.
// ---------------------------------------------------------------------------------------------------------------
struct ManoFitArgs {
  const float *target, *weight;
  const float *vtarget, *vweight;  // [B][778][3] mm, [B][778] >= 0: the vertex term (the instantiation with VT only)
  ManoModel m;
  kpf_mano_fit_cfg c;
  float lambda_verts;
  int res_ld;                      // 2: residual [B][2] (joints before / after); 4: [B][4], the vertex distances before / after in columns 2, 3
  float *pose, *betas, *trans, *verts, *joints, *rotmat, *residual;
  int* status;
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

// VT: with the vertex term.  Without it the kernel is the joint fit as it was: every statement of that path is the one it had, and so are its bits.
template <bool VT>
__global__ __launch_bounds__(256) void mano_fit_kernel(ManoFitArgs a) {
  __shared__ ManoLds s;
  __shared__ ManoGradLds g;
  __shared__ ManoFitLds f;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* vc = VT ? a.vtarget + (long)b * NC : nullptr;
  const float* vu = VT ? a.vweight + (long)b * NV : nullptr;
  if (t < 48) f.P[t] = a.pose[(long)b * 48 + t];
  else if (t < 58) f.P[t] = a.betas[(long)b * 10 + (t - 48)];
  else if (t < 61) f.P[t] = a.trans[(long)b * 3 + (t - 58)];
  if (t < 61) f.M1[t] = f.M2[t] = 0.0f;
  if (t >= 64 && t < 64 + 21) {
    // every sum over the joints below runs in the model's order: a permuted joint_map with equally permuted targets gives the same bits
    const int i = t - 64, h = a.c.joint_map[i];
    const float w = a.target ? (a.weight ? a.weight[(long)b * 21 + i] : 1.0f) : 0.0f;  // no joint targets (the mesh entry allows it): every joint weight is 0
    f.W[h] = w;
    for (int d = 0; d < 3; ++d) f.Y[h][d] = w > 0.0f ? a.target[((long)b * 21 + i) * 3 + d] : 0.0f;  // a target of weight 0 is selected out, not multiplied
  }
  float vstat[2] = {0.f, 0.f};  // sum of the vertex weights, non-finite vertex targets under a positive weight
  if constexpr (VT) {
    float in[2];
    mano_vert_weights(vc, vu, t, in);
    mano_block_sum<2>(f, t, in, vstat);
  }
  __syncthreads();
  if (t == 0) {
    float sw = 0.f;
    int st = 0;
    for (int i = 0; i < 21; ++i) {
      if (!(f.W[i] > 0.0f)) continue;
      sw += f.W[i];
      if (!(isfinite(f.Y[i][0]) && isfinite(f.Y[i][1]) && isfinite(f.Y[i][2]))) st |= 2;
    }
    if (VT && vstat[1] > 0.0f) st |= 2;
    if (!(sw > 0.0f) && !(VT && vstat[0] > 0.0f)) st |= 1;  // with the vertex term: both weight sums are 0
    f.sw = sw;
    f.sv = vstat[0];
    f.status = st;
  }
  __syncthreads();
  const bool ok = f.status == 0;  // otherwise: no init, no iteration, the state keeps its bits and the outputs evaluate it
  const int iters = ok ? a.c.iters : 0;
  mano_fit_eval<VT>(a.m, s, f, g.dv, t);
  if (iters > 0 && a.c.init_trans) {  // "before iteration 1": iters == 0 only evaluates
    if constexpr (!VT) {
      if (t < 3) {
        float sum = 0.f;
        for (int i = 0; i < 21; ++i)
          if (f.W[i] > 0.0f) sum = fmaf(f.W[i], f.Y[i][t] - f.Jm[i][t], sum);
        f.P[58 + t] = sum / f.sw;
      }
    } else if (f.sw > 0.0f) {
      // With the vertex term the mean offset is summed in double and rounded once: at half a metre one float ulp is 6e-5 mm, a sum of 21 such offsets in
      // float is off by about that, and an error of t is the same for every vertex -- it does not average out of the pose gradient as a vertex's own
      // rounding does, and was the largest term of the first step's pose error
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
      mano_vert_offset(vc, vu, g.dv, t, in);
      mano_block_sum3d(f, t, in, off);
      if (t < 3) f.P[58 + t] = (float)((t == 0 ? off[0] : (t == 1 ? off[1] : off[2])) / (double)f.sv);
    }
    __syncthreads();
  }
  if (t == 0) a.residual[(long)b * a.res_ld + 0] = mano_fit_residual(f);
  if constexpr (VT) {
    float in = mano_vert_distance(vc, vu, g.dv, &f.P[58], t), sum;
    mano_block_sum<1>(f, t, &in, &sum);
    if (t == 0) a.residual[(long)b * a.res_ld + 2] = f.sv > 0.0f ? sum / f.sv : 0.0f;
  } else {
    if (t == 0 && a.res_ld == 4) a.residual[(long)b * 4 + 2] = 0.0f;
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
    a.residual[(long)b * a.res_ld + 1] = mano_fit_residual(f);
    a.status[b] = f.status;
  }
  if constexpr (VT) {
    float in = mano_vert_distance(vc, vu, g.dv, &f.P[58], t), sum;
    mano_block_sum<1>(f, t, &in, &sum);
    if (t == 0) a.residual[(long)b * a.res_ld + 3] = f.sv > 0.0f ? sum / f.sv : 0.0f;
  } else {
    if (t == 0 && a.res_ld == 4) a.residual[(long)b * 4 + 3] = 0.0f;
  }
  if (ok) {
    if (t < 48) a.pose[(long)b * 48 + t] = f.P[t];
    else if (t < 58) a.betas[(long)b * 10 + (t - 48)] = f.P[t];
    else if (t < 61) a.trans[(long)b * 3 + (t - 58)] = f.P[t];
  }
  if (t < 63) {
    const int i = t / 3, d = t - i * 3;
    a.joints[((long)b * 21 + i) * 3 + d] = f.Jm[a.c.joint_map[i]][d] + f.P[58 + d];
  }
  if (a.rotmat && t >= 64 && t < 64 + NJ) {  // rodrigues(pose_aa[j]): without hands_mean
    float R[9];
    rodrigues(&f.P[(t - 64) * 3], R);
    for (int i = 0; i < 9; ++i) a.rotmat[((long)b * NJ + (t - 64)) * 9 + i] = R[i];
  }
  if (a.verts)
    for (int v = t; v < NV; v += 256) {
      float o[3];
      mano_skin_vertex(a.m, s, v, o);
#pragma unroll
      for (int r = 0; r < 3; ++r) a.verts[((long)b * NV + v) * 3 + r] = o[r] * 1000.0f + f.P[58 + r];
    }
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
  const float *target, *weight;
  ManoModel m;
  kpf_mano_fit_gn_cfg c;
  float *pose, *betas, *trans, *verts, *joints, *rotmat, *residual;
  int* status;
  float *history, *jacobian;  // [B][iters + 1], [B][63][61]; each may be null
  int res_ld, hist_ld;        // 2 and 1: the layouts above.  4 and 2 (the mesh entry without a vertex term): residual [B][4] and history [B][iters + 1][2],
                              // the vertex distances (columns 2, 3 and entry 1 of each pair) written as 0
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

__global__ __launch_bounds__(256) void mano_fit_gn_kernel(ManoGnArgs a) {
  __shared__ ManoLds s;
  __shared__ ManoFitLds f;
  __shared__ ManoGnLds n;
  const int b = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  // the state, the targets and the status: the Adam fit's text
  if (t < 48) f.P[t] = a.pose[(long)b * 48 + t];
  else if (t < 58) f.P[t] = a.betas[(long)b * 10 + (t - 48)];
  else if (t < 61) f.P[t] = a.trans[(long)b * 3 + (t - 58)];
  if (t >= 64 && t < 64 + 21) {
    const int i = t - 64, h = a.c.joint_map[i];
    const float w = a.weight ? a.weight[(long)b * 21 + i] : 1.0f;
    f.W[h] = w;
    n.inv[h] = i;
    for (int d = 0; d < 3; ++d) f.Y[h][d] = w > 0.0f ? a.target[((long)b * 21 + i) * 3 + d] : 0.0f;  // a target of weight 0 is selected out, not multiplied
  }
  if (t >= 128 && t < 128 + 5 * NJ) n.tipW[(t - 128) / NJ][(t - 128) % NJ] = a.m.skin[(long)kManoTip[(t - 128) / NJ] * NJ + (t - 128) % NJ];
  if (t == 255) n.fail = 0;
  __syncthreads();
  if (t == 0) {
    float sw = 0.f;
    int st = 0;
    for (int i = 0; i < 21; ++i) {
      if (!(f.W[i] > 0.0f)) continue;
      sw += f.W[i];
      if (!(isfinite(f.Y[i][0]) && isfinite(f.Y[i][1]) && isfinite(f.Y[i][2]))) st |= 2;
    }
    if (!(sw > 0.0f)) st |= 1;
    f.sw = sw;
    f.sv = 0.0f;
    f.status = st;
  }
  __syncthreads();
  const bool ok = f.status == 0;  // otherwise: no init, no iteration, the state keeps its bits and the outputs evaluate it
  const int iters = ok ? a.c.iters : 0;
  float* hist = a.history ? a.history + (long)b * (a.c.iters + 1) * a.hist_ld : nullptr;
  float* jac = a.jacobian ? a.jacobian + (long)b * GN_R * GN_P : nullptr;
  if (t < 21) n.SQ[t] = (ok && f.W[t] > 0.0f) ? sqrtf(f.W[t] / f.sw) : 0.0f;
  if (iters > 0 || jac) {  // d Jr / d beta: 48 dot products of length 778 per beta, a wave per beta
    for (int k = wave; k < 10; k += 4) {
      float acc[NJ * 3];
#pragma unroll
      for (int o = 0; o < NJ * 3; ++o) acc[o] = 0.f;
      for (int v = lane; v < NV; v += 64) {
        const float sx = a.m.shapeT[(long)k * NC + v * 3 + 0], sy = a.m.shapeT[(long)k * NC + v * 3 + 1], sz = a.m.shapeT[(long)k * NC + v * 3 + 2];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const float w = a.m.jreg[(long)j * NV + v];
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
  mano_fit_eval<false>(a.m, s, f, nullptr, t);
  if (iters > 0 && a.c.init_trans) {  // summed in double and rounded once, as the mesh fit does
    if (t < 3) {
      double sum = 0.0, den = 0.0;
      for (int i = 0; i < 21; ++i)
        if (f.W[i] > 0.0f) {
          sum = fma((double)f.W[i], (double)f.Y[i][t] - (double)f.Jm[i][t], sum);
          den += (double)f.W[i];
        }
      f.P[58 + t] = (float)(sum / den);
    }
    __syncthreads();
  }
  if (t == 0) a.residual[(long)b * a.res_ld + 0] = mano_fit_residual(f);
  if (iters == 0 && jac) mano_gn_tangent<false>(a.m, s, f, n, t, jac);  // only evaluates: the entry Jacobian is still reported
  int slot[GN_SLOTS];
  mano_gn_slots(t, slot);
  int done = 0, st4 = 0;
  for (int it = 1; it <= iters; ++it) {
    if (it > 1) mano_fit_eval<false>(a.m, s, f, nullptr, t);
    if (t == 0 && hist) hist[(it - 1) * a.hist_ld] = mano_fit_residual(f);
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
    a.residual[(long)b * a.res_ld + 1] = res;
    a.status[b] = f.status | st4;
    if (hist)  // after a stop the state no longer moves: the remaining entries repeat the last one
      for (int it = (st4 ? done : iters); it <= a.c.iters; ++it) hist[it * a.hist_ld] = res;
    if (a.res_ld == 4) a.residual[(long)b * 4 + 2] = a.residual[(long)b * 4 + 3] = 0.0f;
    if (hist && a.hist_ld == 2)
      for (int it = 0; it <= a.c.iters; ++it) hist[it * 2 + 1] = 0.0f;
  }
  if (ok) {
    if (t < 48) a.pose[(long)b * 48 + t] = f.P[t];
    else if (t < 58) a.betas[(long)b * 10 + (t - 48)] = f.P[t];
    else if (t < 61) a.trans[(long)b * 3 + (t - 58)] = f.P[t];
  }
  if (t < 63) {
    const int i = t / 3, d = t - i * 3;
    a.joints[((long)b * 21 + i) * 3 + d] = f.Jm[a.c.joint_map[i]][d] + f.P[58 + d];
  }
  if (a.rotmat && t >= 64 && t < 64 + NJ) {  // rodrigues(pose_aa[j]): without hands_mean
    float R[9];
    rodrigues(&f.P[(t - 64) * 3], R);
    for (int i = 0; i < 9; ++i) a.rotmat[((long)b * NJ + (t - 64)) * 9 + i] = R[i];
  }
  if (a.verts)
    for (int v = t; v < NV; v += 256) {
      float o[3];
      mano_skin_vertex(a.m, s, v, o);
#pragma unroll
      for (int r = 0; r < 3; ++r) a.verts[((long)b * NV + v) * 3 + r] = o[r] * 1000.0f + f.P[58 + r];
    }
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
  const float *target, *weight, *vtarget, *vweight;  // target may be null (no joint carries weight); the vertex pair is never null here
  ManoModel m;
  kpf_mano_fit_gn_cfg c;
  float lambda_verts;
  float *pose, *betas, *trans, *verts, *joints, *rotmat, *residual;
  int* status;
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
  // the state, the targets and the status: the mesh fit's rules
  if (t < 48) f.P[t] = a.pose[(long)b * 48 + t];
  else if (t < 58) f.P[t] = a.betas[(long)b * 10 + (t - 48)];
  else if (t < 61) f.P[t] = a.trans[(long)b * 3 + (t - 58)];
  if (t >= 64 && t < 64 + 21) {
    const int i = t - 64, h = a.c.joint_map[i];
    const float w = a.target ? (a.weight ? a.weight[(long)b * 21 + i] : 1.0f) : 0.0f;
    f.W[h] = w;
    n.inv[h] = i;
    for (int d = 0; d < 3; ++d) f.Y[h][d] = w > 0.0f ? a.target[((long)b * 21 + i) * 3 + d] : 0.0f;  // a target of weight 0 is selected out, not multiplied
  }
  if (t >= 128 && t < 128 + 5 * NJ) n.tipW[(t - 128) / NJ][(t - 128) % NJ] = a.m.skin[(long)kManoTip[(t - 128) / NJ] * NJ + (t - 128) % NJ];
  if (t == 255) n.fail = 0;
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
  __syncthreads();
  if (t == 0) {
    float sw = 0.f;
    int st = 0;
    for (int i = 0; i < 21; ++i) {
      if (!(f.W[i] > 0.0f)) continue;
      sw += f.W[i];
      if (!(isfinite(f.Y[i][0]) && isfinite(f.Y[i][1]) && isfinite(f.Y[i][2]))) st |= 2;
    }
    if (vstat[1] > 0.0f) st |= 2;
    if (!(sw > 0.0f) && !(vstat[0] > 0.0f)) st |= 1;
    f.sw = sw;
    f.sv = vstat[0];
    f.status = st;
  }
  __syncthreads();
  const bool ok = f.status == 0;  // otherwise: no init, no iteration, the state keeps its bits and the outputs evaluate it
  const int iters = ok ? a.c.iters : 0;
  float* hist = a.history ? a.history + (long)b * (a.c.iters + 1) * 2 : nullptr;
  float* jac = a.jacobian ? a.jacobian + (long)b * GN_R * GN_P : nullptr;
  float* vjac = a.vjacobian ? a.vjacobian + (long)b * NC * GN_P : nullptr;
  if (t < 21) n.SQ[t] = (ok && f.W[t] > 0.0f) ? sqrtf(f.W[t] / f.sw) : 0.0f;
  if (iters > 0 || jac || vjac) {  // d Jr / d beta, as the joint fit forms it
    for (int k = wave; k < 10; k += 4) {
      float acc[NJ * 3];
#pragma unroll
      for (int o = 0; o < NJ * 3; ++o) acc[o] = 0.f;
      for (int v = lane; v < NV; v += 64) {
        const float sx = a.m.shapeT[(long)k * NC + v * 3 + 0], sy = a.m.shapeT[(long)k * NC + v * 3 + 1], sz = a.m.shapeT[(long)k * NC + v * 3 + 2];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const float w = a.m.jreg[(long)j * NV + v];
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
  mano_fit_eval<true>(a.m, s, f, x.vm, t);
  if (iters > 0 && a.c.init_trans) {  // the mesh fit's rule: from the joints when they carry weight, otherwise from the vertices; in double, rounded once
    if (f.sw > 0.0f) {
      if (t < 3) {
        double sum = 0.0, den = 0.0;
        for (int i = 0; i < 21; ++i)
          if (f.W[i] > 0.0f) {
            sum = fma((double)f.W[i], (double)f.Y[i][t] - (double)f.Jm[i][t], sum);
            den += (double)f.W[i];
          }
        f.P[58 + t] = (float)(sum / den);
      }
    } else {
      double in[3], off[3];
      mano_vert_offset(x.c, x.u, x.vm, t, in);
      mano_block_sum3d(f, t, in, off);
      if (t < 3) f.P[58 + t] = (float)((t == 0 ? off[0] : (t == 1 ? off[1] : off[2])) / (double)f.sv);
    }
    __syncthreads();
  }
  {
    const float dv = mano_mesh_gn_vert_distance<PLANE>(f, x, vn, t);
    if (t == 0) {
      a.residual[(long)b * 4 + 0] = mano_fit_residual(f);
      a.residual[(long)b * 4 + 2] = dv;
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
      if (t == 0) {
        hist[(it - 1) * 2 + 0] = mano_fit_residual(f);
        hist[(it - 1) * 2 + 1] = dv;
      }
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
      a.residual[(long)b * 4 + 1] = res;
      a.residual[(long)b * 4 + 3] = dv;
      a.status[b] = f.status | st4;
      if (hist)  // after a stop the state no longer moves: the remaining entries repeat the last one
        for (int it = (st4 ? done : iters); it <= a.c.iters; ++it) {
          hist[it * 2 + 0] = res;
          hist[it * 2 + 1] = dv;
        }
    }
  }
  if (ok) {
    if (t < 48) a.pose[(long)b * 48 + t] = f.P[t];
    else if (t < 58) a.betas[(long)b * 10 + (t - 48)] = f.P[t];
    else if (t < 61) a.trans[(long)b * 3 + (t - 58)] = f.P[t];
  }
  if (t < 63) {
    const int i = t / 3, d = t - i * 3;
    a.joints[((long)b * 21 + i) * 3 + d] = f.Jm[a.c.joint_map[i]][d] + f.P[58 + d];
  }
  if (a.rotmat && t >= 64 && t < 64 + NJ) {  // rodrigues(pose_aa[j]): without hands_mean
    float R[9];
    rodrigues(&f.P[(t - 64) * 3], R);
    for (int i = 0; i < 9; ++i) a.rotmat[((long)b * NJ + (t - 64)) * 9 + i] = R[i];
  }
  if (a.verts)
    for (int c = t; c < NC; c += 256) a.verts[(long)b * NC + c] = x.vm[c] + f.P[58 + c % 3];
}

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
  {  // this thread's vertices t, t + 256, t + 512, (t + 768): one pass over the points in ascending order serves all of them
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
      a.vweight[(long)b * NV + v] = any ? W[k] : 0.0f;
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vtarget[((long)b * NV + v) * 3 + d] = any ? __fdiv_rn(S[k][d], W[k]) : 0.0f;
    }
  }
  if (t == 255) {  // the matched points' count and mean distance, summed in ascending point order
    float sum = 0.f;
    int cnt = 0;
    for (int n = 0; n < N; ++n)
      if (s.idx[n] >= 0) {
        sum = __fadd_rn(sum, s.dist[n]);
        ++cnt;
      }
    a.stats[(long)b * 2 + 0] = (float)cnt;
    a.stats[(long)b * 2 + 1] = cnt > 0 ? __fdiv_rn(sum, (float)cnt) : 0.0f;
  }
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
  {  // this thread's vertices t, t + 256, t + 512, (t + 768): one pass over the points in ascending order serves all of them
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
      a.vweight[(long)b * NV + v] = any ? W[k] : 0.0f;
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vtarget[((long)b * NV + v) * 3 + d] = any ? __fdiv_rn(S[k][d], W[k]) : 0.0f;
    }
  }
  if (t == 255) {  // the matched points' count and mean distances, summed in ascending point order; the visible vertices
    float sum = 0.f, psum = 0.f;
    int cnt = 0;
    for (int n = 0; n < N; ++n)
      if (s.idx[n] >= 0) {
        sum = __fadd_rn(sum, s.dist[n]);
        psum = __fadd_rn(psum, s.plane[n]);
        ++cnt;
      }
    a.stats[(long)b * 4 + 0] = (float)cnt;
    a.stats[(long)b * 4 + 1] = cnt > 0 ? __fdiv_rn(sum, (float)cnt) : 0.0f;
    a.stats[(long)b * 4 + 2] = cnt > 0 ? __fdiv_rn(psum, (float)cnt) : 0.0f;
    a.stats[(long)b * 4 + 3] = (float)nvis;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// z-buffer render of the mesh into the crop's pixel grid: depth, the owning face, the vertices that lie behind another part of the mesh
// along their pixel's ray, and the comparison with an observed depth crop.  One workgroup per hand; the z-buffer is H * W 64-bit words of LDS holding
// (bits(d) << 32) | face, and a face's candidate enters by an integer min: a positive float's bits order as the float does, so the smallest depth wins, among
// equal depths the lowest face, whatever the order the faces arrive in.  A thread owns faces t, t + 256, ...: it walks a pixel box of up to
// RASTER_SMALL pixels itself and queues a larger face, which a whole wave then walks, 8 x 8 pixels at a step (the queue's order does not matter either).
// The faces are read from global memory (at 128 x 128 the buffer alone is 131072 of the 163840 bytes).  There is no near-plane clipping: a face with a vertex at z <= 0 is
// skipped whole.  Every operation individually rounded: tests/mano_raster_cases.py::raster_host gives the same bits.
// ---------------------------------------------------------------------------------------------------------------
constexpr int RASTER_MAXPIX = 16384;
constexpr unsigned long long RASTER_EMPTY = ~0ull;
constexpr int RASTER_SMALL = 64;

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

// One directed edge a -> b, always evaluated from the lower vertex index: e = (sx[hi] - sx[lo]) (py - sy[lo]) - (sy[hi] - sy[lo]) (px - sx[lo]), negated
// if a > b.  The two faces at an edge get the same number with opposite signs, so with an inclusive test a pixel centre on the edge belongs to one of them.
struct RasterEdge {
  float dx, dy, ox, oy;
  bool neg;
  __device__ __forceinline__ void set(const float* sx, const float* sy, int a, int b) {
#pragma clang fp contract(off)
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    dx = __fsub_rn(sx[hi], sx[lo]);
    dy = __fsub_rn(sy[hi], sy[lo]);
    ox = sx[lo];
    oy = sy[lo];
    neg = a > b;
  }
  __device__ __forceinline__ float at(float px, float py) const {
#pragma clang fp contract(off)
    const float e = __fsub_rn(__fmul_rn(dx, __fsub_rn(py, oy)), __fmul_rn(dy, __fsub_rn(px, ox)));
    return neg ? -e : e;
  }
};

// One face ready to be walked: its three edges (w0, w1, w2 are the weights of v0, v1, v2), the vertices' 1 / z, the sign of its area and its pixel box
struct RasterFace {
  RasterEdge e0, e1, e2;
  float iz0, iz1, iz2;
  bool pos;
  int x0, x1, y0, y1;
  // false: the face is skipped (an index outside 0..777, a repeated one, a vertex that is not finite or has z <= 0, no area, no pixel)
  __device__ __forceinline__ bool set(const int* faces, int k, const float* sx, const float* sy, const float* iz, const int* ok, int H, int W) {
#pragma clang fp contract(off)
    const int i0 = faces[k * 3 + 0], i1 = faces[k * 3 + 1], i2 = faces[k * 3 + 2];
    if ((unsigned)i0 >= (unsigned)NV || (unsigned)i1 >= (unsigned)NV || (unsigned)i2 >= (unsigned)NV) return false;
    if (i0 == i1 || i1 == i2 || i0 == i2) return false;
    if (!(ok[i0] && ok[i1] && ok[i2])) return false;
    e0.set(sx, sy, i1, i2);
    e1.set(sx, sy, i2, i0);
    e2.set(sx, sy, i0, i1);
    const float area = e2.at(sx[i2], sy[i2]);
    if (area == 0.0f || !isfinite(area)) return false;  // a finite area: every sx, sy of the face is finite
    // the pixel box, clamped to the window in float: a vertex at z = 1e-3 mm projects to 1e9
    const float x0f = fmaxf(ceilf(fminf(fminf(sx[i0], sx[i1]), sx[i2])), 0.0f), x1f = fminf(floorf(fmaxf(fmaxf(sx[i0], sx[i1]), sx[i2])), (float)(W - 1));
    const float y0f = fmaxf(ceilf(fminf(fminf(sy[i0], sy[i1]), sy[i2])), 0.0f), y1f = fminf(floorf(fmaxf(fmaxf(sy[i0], sy[i1]), sy[i2])), (float)(H - 1));
    if (!(x0f <= x1f && y0f <= y1f)) return false;
    x0 = (int)x0f; x1 = (int)x1f; y0 = (int)y0f; y1 = (int)y1f;  // inside [0, W - 1] x [0, H - 1]
    iz0 = iz[i0]; iz1 = iz[i1]; iz2 = iz[i2];
    pos = area > 0.0f;
    return true;
  }
  // pixel (c, r) of the box: the face's depth there enters the z-buffer if the pixel centre is inside
  __device__ __forceinline__ void pixel(int c, int r, int k, unsigned long long* zb, int W) const {
#pragma clang fp contract(off)
    const float px = (float)c, py = (float)r;
    const float w0 = e0.at(px, py), w1 = e1.at(px, py), w2 = e2.at(px, py);
    const bool in = pos ? (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) : (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);  // two-sided: MANO is open at the wrist
    if (!in) return;
    const float sum = __fadd_rn(__fadd_rn(w0, w1), w2);
    const float izp = __fadd_rn(__fadd_rn(__fmul_rn(__fdiv_rn(w0, sum), iz0), __fmul_rn(__fdiv_rn(w1, sum), iz1)), __fmul_rn(__fdiv_rn(w2, sum), iz2));
    const float d = __fdiv_rn(1.0f, izp);  // perspective-correct
    if (isfinite(d) && d > 0.0f) atomicMin(&zb[r * W + c], ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)k);
  }
};

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
    if (!f.set(a.faces, k, sx, sy, iz, ok, H, W)) continue;
    if ((f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) > RASTER_SMALL) {
      queue[atomicAdd(&count[3], 1)] = (unsigned short)k;
      continue;
    }
    for (int r = f.y0; r <= f.y1; ++r)
      for (int c = f.x0; c <= f.x1; ++c) f.pixel(c, r, k, zb, W);
  }
  __syncthreads();
  for (int q = t >> 6; q < count[3]; q += 4) {  // a queued face is walked by one wave, 8 x 8 pixels at a step
    const int k = queue[q];
    RasterFace f;
    f.set(a.faces, k, sx, sy, iz, ok, H, W);
    for (int r = f.y0 + ((t & 63) >> 3); r <= f.y1; r += 8)
      for (int c = f.x0 + (t & 7); c <= f.x1; c += 8) f.pixel(c, r, k, zb, W);
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

extern "C" int kpf_mano_forward_f32(const float* pose6d, int ld6, const float* betas, int ldb, const float* shapedirs_t,
                                    const float* posedirs_t, const float* v_template, const float* j_regressor, const float* skin_weights,
                                    const float* hands_mean, float* verts, float* joints, float* rotmat, float* pose_aa, int B,
                                    void* stream) {
  KPF_REQUIRE(pose6d && betas && shapedirs_t && posedirs_t && v_template && j_regressor && skin_weights && hands_mean && verts && joints &&
                  rotmat && pose_aa,
              "kpf_mano_forward_f32: null pointer");
  KPF_REQUIRE(B > 0 && ld6 >= 96 && ldb >= 10, "kpf_mano_forward_f32: bad shape B=%d ld6=%d ldb=%d", B, ld6, ldb);
  ManoArgs a;
  a.pose6d = pose6d; a.betas = betas; a.ld6 = ld6; a.ldb = ldb;
  a.m = ManoModel{shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean};
  a.verts = verts; a.joints = joints; a.rotmat = rotmat; a.aa = pose_aa;
  hipLaunchKernelGGL(mano_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch("kpf_mano_forward_f32");
}

extern "C" int kpf_mano_backward_f32(const float* pose6d, int ld6, const float* betas, int ldb, const float* shapedirs_t,
                                     const float* posedirs_t, const float* v_template, const float* j_regressor, const float* skin_weights,
                                     const float* hands_mean, const float* d_verts, const float* d_joints, const float* d_rotmat,
                                     const float* d_pose_aa, float* d_pose6d, int ldd6, float* d_betas, int lddb, int B, void* stream) {
  KPF_REQUIRE(pose6d && betas && shapedirs_t && posedirs_t && v_template && j_regressor && skin_weights && hands_mean && d_pose6d && d_betas,
              "kpf_mano_backward_f32: null pointer");
  KPF_REQUIRE(B > 0 && ld6 >= 96 && ldb >= 10 && ldd6 >= 96 && lddb >= 10, "kpf_mano_backward_f32: bad shape B=%d ld6=%d ldb=%d ldd6=%d lddb=%d", B, ld6,
              ldb, ldd6, lddb);
  ManoBwdArgs a;
  a.pose6d = pose6d; a.betas = betas; a.ld6 = ld6; a.ldb = ldb;
  a.m = ManoModel{shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean};
  a.d_verts = d_verts; a.d_joints = d_joints; a.d_rotmat = d_rotmat; a.d_aa = d_pose_aa;
  a.d_pose6d = d_pose6d; a.d_betas = d_betas; a.ldd6 = ldd6; a.lddb = lddb;
  hipLaunchKernelGGL(mano_backward_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch("kpf_mano_backward_f32");
}

// The two fit entries: `name` prefixes every refusal; vert_target / vert_weight select the instantiation with the vertex term
static int mano_fit_launch(const char* name, const float* target, const float* weight, const float* vert_target, const float* vert_weight,
                           const float* shapedirs_t, const float* posedirs_t, const float* v_template, const float* j_regressor, const float* skin_weights,
                           const float* hands_mean, const kpf_mano_fit_cfg* cfg, float lambda_verts, float* pose_aa, float* betas, float* trans, float* verts,
                           float* joints, float* rotmat, float* residual, int res_ld, int* status, int B, void* stream) {
  KPF_REQUIRE(shapedirs_t && posedirs_t && v_template && j_regressor && skin_weights && hands_mean && cfg && pose_aa && betas && trans && joints &&
                  residual && status,
              "%s: null pointer", name);
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  KPF_REQUIRE(cfg->iters >= 0 && cfg->iters <= 1000, "%s: iters=%d outside [0, 1000]", name, cfg->iters);
  KPF_REQUIRE(cfg->beta1 >= 0.f && cfg->beta1 < 1.f && cfg->beta2 >= 0.f && cfg->beta2 < 1.f && cfg->eps >= 0.f,
              "%s: bad Adam constants beta1=%g beta2=%g eps=%g", name, cfg->beta1, cfg->beta2, cfg->eps);
  unsigned seen = 0;
  for (int i = 0; i < 21; ++i) {
    KPF_REQUIRE(cfg->joint_map[i] >= 0 && cfg->joint_map[i] < 21, "%s: joint_map[%d]=%d outside [0, 21)", name, i, cfg->joint_map[i]);
    seen |= 1u << cfg->joint_map[i];
  }
  KPF_REQUIRE(seen == (1u << 21) - 1, "%s: joint_map is not a permutation", name);
  ManoFitArgs a;
  a.target = target; a.weight = weight; a.vtarget = vert_target; a.vweight = vert_weight;
  a.m = ManoModel{shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean};
  a.c = *cfg;
  a.lambda_verts = lambda_verts; a.res_ld = res_ld;
  a.pose = pose_aa; a.betas = betas; a.trans = trans; a.verts = verts; a.joints = joints; a.rotmat = rotmat; a.residual = residual;
  a.status = status;
  if (vert_target && vert_weight) hipLaunchKernelGGL(mano_fit_kernel<true>, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(mano_fit_kernel<false>, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

extern "C" int kpf_mano_fit_f32(const float* target, const float* weight, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                                const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_cfg* cfg,
                                float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                                int B, void* stream) {
  KPF_REQUIRE(target, "kpf_mano_fit_f32: null pointer");
  return mano_fit_launch("kpf_mano_fit_f32", target, weight, nullptr, nullptr, shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean, cfg,
                         0.0f, pose_aa, betas, trans, verts, joints, rotmat, residual, 2, status, B, stream);
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
  return mano_fit_launch("kpf_mano_fit_mesh_f32", target, weight, vert_target, vert_weight, shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights,
                         hands_mean, &c, cfg->lambda_verts, pose_aa, betas, trans, verts, joints, rotmat, residual, 4, status, B, stream);
}

extern "C" int kpf_mano_fit_gn_f32(const float* target, const float* weight, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                                   const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_gn_cfg* cfg,
                                   float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                                   float* history, float* jacobian, int B, void* stream) {
  const char* name = "kpf_mano_fit_gn_f32";
  KPF_REQUIRE(target && shapedirs_t && posedirs_t && v_template && j_regressor && skin_weights && hands_mean && cfg && pose_aa && betas && trans && joints &&
                  residual && status,
              "%s: null pointer", name);
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  KPF_REQUIRE(cfg->iters >= 0 && cfg->iters <= 64, "%s: iters=%d outside [0, 64]", name, cfg->iters);
  KPF_REQUIRE(cfg->mu >= 0.f && cfg->nu >= 0.f && isfinite(cfg->mu) && isfinite(cfg->nu), "%s: bad damping mu=%g nu=%g", name, cfg->mu, cfg->nu);
  unsigned seen = 0;
  for (int i = 0; i < 21; ++i) {
    KPF_REQUIRE(cfg->joint_map[i] >= 0 && cfg->joint_map[i] < 21, "%s: joint_map[%d]=%d outside [0, 21)", name, i, cfg->joint_map[i]);
    seen |= 1u << cfg->joint_map[i];
  }
  KPF_REQUIRE(seen == (1u << 21) - 1, "%s: joint_map is not a permutation", name);
  ManoGnArgs a;
  a.target = target; a.weight = weight;
  a.m = ManoModel{shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean};
  a.c = *cfg;
  a.pose = pose_aa; a.betas = betas; a.trans = trans; a.verts = verts; a.joints = joints; a.rotmat = rotmat; a.residual = residual;
  a.status = status; a.history = history; a.jacobian = jacobian;
  a.res_ld = 2; a.hist_ld = 1;
  hipLaunchKernelGGL(mano_fit_gn_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

// The two Gauss-Newton mesh entries: `name` prefixes every refusal; vert_normal selects the instantiation with the point-to-plane vertex term
static int mano_mesh_gn_launch(const char* name, const float* target, const float* weight, const float* vert_target, const float* vert_weight,
                               const float* vert_normal, const float* shapedirs_t, const float* posedirs_t, const float* v_template,
                               const float* j_regressor, const float* skin_weights, const float* hands_mean, const kpf_mano_fit_mesh_gn_cfg* cfg,
                               float* pose_aa, float* betas, float* trans, float* verts, float* joints, float* rotmat, float* residual, int* status,
                               float* history, float* jacobian, float* vert_jacobian, int B, void* stream) {
  KPF_REQUIRE(shapedirs_t && posedirs_t && v_template && j_regressor && skin_weights && hands_mean && cfg && pose_aa && betas && trans && joints &&
                  residual && status,
              "%s: null pointer", name);
  KPF_REQUIRE((vert_target == nullptr) == (vert_weight == nullptr), "%s: vert_target and vert_weight go together", name);
  KPF_REQUIRE(target || vert_target, "%s: neither joint nor vertex targets", name);
  KPF_REQUIRE(vert_target || !vert_jacobian, "%s: vert_jacobian needs the vertex term", name);
  KPF_REQUIRE(vert_target || !vert_normal, "%s: vert_normal needs the vertex term", name);
  KPF_REQUIRE(B > 0, "%s: bad shape B=%d", name, B);
  KPF_REQUIRE(cfg->iters >= 0 && cfg->iters <= 64, "%s: iters=%d outside [0, 64]", name, cfg->iters);
  KPF_REQUIRE(cfg->mu >= 0.f && cfg->nu >= 0.f && isfinite(cfg->mu) && isfinite(cfg->nu), "%s: bad damping mu=%g nu=%g", name, cfg->mu, cfg->nu);
  KPF_REQUIRE(cfg->lambda_verts >= 0.f && isfinite(cfg->lambda_verts), "%s: lambda_verts=%g is negative or not finite", name, cfg->lambda_verts);
  unsigned seen = 0;
  for (int i = 0; i < 21; ++i) {
    KPF_REQUIRE(cfg->joint_map[i] >= 0 && cfg->joint_map[i] < 21, "%s: joint_map[%d]=%d outside [0, 21)", name, i, cfg->joint_map[i]);
    seen |= 1u << cfg->joint_map[i];
  }
  KPF_REQUIRE(seen == (1u << 21) - 1, "%s: joint_map is not a permutation", name);
  kpf_mano_fit_gn_cfg c;
  c.iters = cfg->iters;
  c.mu = cfg->mu; c.nu = cfg->nu;
  c.lambda_shape = cfg->lambda_shape; c.lambda_pose = cfg->lambda_pose;
  c.init_trans = cfg->init_trans;
  for (int i = 0; i < 21; ++i) c.joint_map[i] = cfg->joint_map[i];
  const ManoModel m{shapedirs_t, posedirs_t, v_template, j_regressor, skin_weights, hands_mean};
  if (!vert_target) {  // no vertex term: the joint fit's kernel, its bits
    ManoGnArgs a;
    a.target = target; a.weight = weight;
    a.m = m;
    a.c = c;
    a.pose = pose_aa; a.betas = betas; a.trans = trans; a.verts = verts; a.joints = joints; a.rotmat = rotmat; a.residual = residual;
    a.status = status; a.history = history; a.jacobian = jacobian;
    a.res_ld = 4; a.hist_ld = 2;
    hipLaunchKernelGGL(mano_fit_gn_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return kpf_check_launch(name);
  }
  ManoMeshGnArgs a;
  a.target = target; a.weight = weight; a.vtarget = vert_target; a.vweight = vert_weight;
  a.m = m;
  a.c = c;
  a.lambda_verts = cfg->lambda_verts;
  a.pose = pose_aa; a.betas = betas; a.trans = trans; a.verts = verts; a.joints = joints; a.rotmat = rotmat; a.residual = residual;
  a.status = status; a.history = history; a.jacobian = jacobian; a.vjacobian = vert_jacobian;
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
