// The MANO hand model (model/mano_head.py:144-225, util/manopth/manopth/manolayer.py:106-273), one 256-thread workgroup per sample:
//   kpf_mano_forward_f32   6D rotations + betas -> vertices, joints, rotations, axis-angle            (eval path of heads.ManoHeadPlan)
//   kpf_mano_backward_f32  its derivative: recomputes the forward in LDS, then walks the stages backwards (heads_train.ManoLayerHip)
// The stage functions are in kpf_mano_dev.h, shared with the fits (kpf_mano_fit.hip); the surface entries are in kpf_mano_surface.hip.  The forward's
// arithmetic is the text it had in kpf_aux.hip (tests/test_heads_gpu.py pins its bits).
// Every reduction has a fixed order (wave butterflies, then a fixed sum over the four waves) and there are no atomics: a replay is bit-identical and a
// sample's bits do not depend on B or on its position in the batch.
#include "kpf_mano_dev.h"

namespace {

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
