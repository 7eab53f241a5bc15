// What the three MANO translation units share (kpf_mano.hip: the layer; kpf_mano_fit.hip: the fits; kpf_mano_surface.hip: association, normals, raster):
// the model's constants, ManoModel, ManoLds, the rotation helpers and their derivatives, mano_blend_chain, the skinning, and mano_backward_lds.  Private to
// csrc; everything is in an unnamed namespace, so each unit compiles its own copy and nothing is exported.
#pragma once
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

}  // namespace
