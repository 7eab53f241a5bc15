// Tracking step behind the forward (keypointfusion_amd/tracking.py): the joints of frame t give the bounding box of frame t + 1 in device memory, so a video
// stream is one captured graph per frame with only the frames uploaded.  One launch, one wave64 per sample, one lane per joint (J <= 64), grid = B; no
// allocation, no synchronisation, no atomics.
//
//   joints (normalised to the cube) -> crop pixels, frame pixels (kpf_uncrop_joint: the bits of kpf_prep_uncrop_f32) and camera-space mm
//   min / max of the STORED float32 frame u, v over the joints: xor butterflies, lanes >= J hold +-inf (min and max do not depend on the order)
//   lane 0: the reference loader's box rule (dataloader/loader.py get_bbox with expansion e in float32, every operation rounded; process_bbox with expansion 1
//   and aspect ratio 1 in float64) = tracking.next_bbox, the host yardstick, bit for bit; then the state: box, seed, lost counter
//
// The whole file is compiled with floating-point contraction OFF (the Makefile's -ffp-contract=on would fuse the float32 steps of the rule, which numpy rounds
// one by one).
#include "kpf_common.h"

#include "kpf_box_dev.h"

#pragma clang fp contract(off)

namespace {

#ifdef __HIPCC__
__device__ __forceinline__ float track_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float track_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(64) void track_step_kernel(const float* __restrict__ joints, const float* __restrict__ center, const float* __restrict__ M,
                                                        const float* __restrict__ cube, const float* __restrict__ cam, const int* __restrict__ pcl_count, int J,
                                                        int frame_w, int frame_h, float expansion, long long seed_stride, double* __restrict__ bbox,
                                                        long long* __restrict__ seed, int* __restrict__ lost, float* __restrict__ crop_px,
                                                        float* __restrict__ frame_px, float* __restrict__ cam_mm, double* __restrict__ bbox_used,
                                                        int* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float inf = __builtin_inff();
  float ulo = inf, uhi = -inf, vlo = inf, vhi = -inf;
  bool bad = false;
  if (lane < J) {
    const size_t e = (size_t)b * J + lane;
    float c3[3], f3[3];
    kpf_uncrop_joint(joints + 3 * e, center + 3 * b, M + 9 * b, cube + 3 * b, cam + 4 * b, c3, f3);
    for (int k = 0; k < 3; ++k) {
      crop_px[3 * e + k] = c3[k];
      frame_px[3 * e + k] = f3[k];
      cam_mm[3 * e + k] = ((joints[3 * e + k] * cube[3 * b + k]) / 2.0f) + center[3 * b + k];  // demo_RGBD.py:133 in float32, each step rounded
    }
    ulo = uhi = f3[0];
    vlo = vhi = f3[1];
    bad = !(isfinite(f3[0]) && isfinite(f3[1]));
  }
  const bool any_bad = __any(bad) != 0;
  ulo = track_wave_min(ulo);
  uhi = track_wave_max(uhi);
  vlo = track_wave_min(vlo);
  vhi = track_wave_max(vhi);
  if (lane != 0) return;

  double box[4];
  for (int k = 0; k < 4; ++k) {
    box[k] = bbox[4 * b + k];
    bbox_used[4 * b + k] = box[k];
  }
  int st = 0;
  if (pcl_count[b] == 0) st |= 2;
  if (any_bad) {
    st |= 4;
  } else {
    if (!kpf_next_box(ulo, uhi, vlo, vhi, expansion, frame_w, frame_h, box)) st |= 1;  // (kpf_box_dev.h: the rule, shared with kpf_detect_hands_u16)
  }
  status[b] = st;
  if (st == 0) {
    for (int k = 0; k < 4; ++k) bbox[4 * b + k] = box[k];
    lost[b] = 0;
  } else {
    lost[b] = lost[b] + 1;  // the box stays what it was
  }
  seed[b] = seed[b] + seed_stride;
}
#endif  // __HIPCC__

}  // namespace

extern "C" int kpf_track_step_f32(const float* joints, const float* center, const float* M, const float* cube, const float* cam_para, const int* pcl_count, int B,
                                  int J, int frame_w, int frame_h, float expansion, long long seed_stride, double* bbox, long long* seed, int* lost,
                                  float* crop_px, float* frame_px, float* cam_mm, double* bbox_used, int* status, void* stream) {
  KPF_REQUIRE(joints && center && M && cube && cam_para && pcl_count && bbox && seed && lost && crop_px && frame_px && cam_mm && bbox_used && status,
              "kpf_track_step_f32: null pointer argument");
  KPF_REQUIRE(B > 0 && J > 0 && frame_w > 0 && frame_h > 0, "kpf_track_step_f32: bad shape (B %d, J %d, frame %d x %d)", B, J, frame_w, frame_h);
  KPF_REQUIRE(J <= 64, "kpf_track_step_f32: J = %d joints (one lane of a wave64 per joint: J <= 64)", J);
  KPF_REQUIRE(expansion > 0.0f && expansion < 1e6f, "kpf_track_step_f32: expansion %g (a positive factor, 1.5 in the reference's loader)", (double)expansion);
  hipLaunchKernelGGL(track_step_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), joints, center, M, cube, cam_para, pcl_count, J, frame_w,
                     frame_h, expansion, seed_stride, bbox, seed, lost, crop_px, frame_px, cam_mm, bbox_used, status);
  return kpf_check_launch("kpf_track_step_f32");
}
