// Device-side RGB-D preprocessing (keypointfusion_amd/preprocess.py on the GPU): frames and boxes in, the model's seven inputs out, and the un-crop of
// the predicted joints.  Three launches, one workgroup per sample (kpf_prep_uncrop_f32: one thread per joint), fixed grids, no host synchronisation:
//
//   kpf_prep_crop_u16    box -> centre of mass (exact 64-bit integer sums, finished by one lane in double) -> metric bounds -> nearest-neighbour crop with
//                        zero padding -> z-clamp -> normalised depth image and RGB crop, plus center / M / cube / cam_para
//                        (kpf_prep_crop_u16_indexed: the same kernel, sample b reading stored frame frame_index[b] — several tracks on one frame)
//   kpf_prep_pcl_sample  foreground pixels of the normalised crop -> candidate points in np.where order -> n of them without replacement IN RANDOM ORDER:
//                        (hash key, candidate) pairs sorted by a bitonic network in LDS (only those under a threshold that about 1.5 n pass), the first n taken
//   kpf_prep_uncrop_f32  normalised joints -> crop pixels -> frame pixels
//   kpf_prep_annot_u16   the crop by the DATASET protocol (preprocess.prepare_annotated): the centre from the annotated joints (or given), left hands mirrored,
//                        float32 up to the integer bounds, plus the labels joint / joint_img; then the same gather and normalisation as kpf_prep_crop_u16
//                        (kpf_prep_uncrop_mirror_f32: the un-crop that takes a mirrored sample's u back to the camera's frame)
//   kpf_prep_augment_u16 the TRAINING item of the dataset protocol (preprocess.prepare_augmented): kpf_prep_annot_u16's crop, then the reference's augmentation
//                        (rotation, centre jitter, cube scale, none; colour scale) of both crops through one inverse map per sample, and of the labels
//   kpf_prep_aug_draw    the augmentation parameters from a device-resident seed (preprocess.draw_augment), which it advances
//
// The host path is the yardstick (tests/test_preprocess_gpu.py): integer decisions and both images are bit-equal to it.  Everything that decides an integer
// is computed in double in the HOST'S operation order, and the whole file is compiled with floating-point contraction OFF (the Makefile's -ffp-contract=on
// would fuse `a * b + c`, which numpy rounds twice); float32 divisions are IEEE divisions.
//
// The three crop kernels (prep_crop_kernel, prep_annot_kernel, prep_augment_kernel) are three launches and share their steps as functions: prep_frame (the
// stored frame of a sample), prep_publish (the per-sample small outputs, from one lane), prep_gather (the z-clamped crop into LDS), prep_normalize_f32 (the
// normalize_depth rule), the LDS plans PREP_LDS_* (read by a kernel and by its launcher) and prep_crop_args (the launchers' common argument checks); the two
// dataset kernels also annot_joint_xyz, annot_centre_geom and prep_label_to_image (normalised label -> joint_img).
#include "kpf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PREP_NT = 1024;  // threads per sample: 16 waves on one CU
constexpr int PREP_NW = PREP_NT / 64;
constexpr int PREP_MAX_PIX = 16384;  // S * S: a candidate index and a pixel index take 14 bits each of a sort element

// ---- preprocess.center_from_bbox: the box in integer pixels, clipped to the frame like a numpy slice (negative corners, which numpy would wrap, clip to 0)
struct PrepBox {
  int x0, x1, y0, y1;  // clipped: columns [x0, x1), rows [y0, y1)
};
__host__ __device__ inline PrepBox prep_box(const double* bbox, int H, int W) {
  const int bx0 = (int)bbox[0], bx1 = (int)(bbox[0] + bbox[2]), by0 = (int)bbox[1], by1 = (int)(bbox[1] + bbox[3]);
  PrepBox r;
  r.x0 = min(max(bx0, 0), W);
  r.x1 = min(max(bx1, r.x0), W);
  r.y0 = min(max(by0, 0), H);
  r.y1 = min(max(by1, r.y0), H);
  return r;
}

struct PrepGeom {
  double com[3];                   // centre of mass (u, v, d mm)
  int xs, xe, ys, ye;              // com_to_bounds
  int szw, szh, offx, offy;        // resize size (w, h) and letterbox offsets inside the S x S crop
  double zs, ze;                   // z range of the cube
  double stepx, stepy;             // resize_nearest: source pixels per destination pixel
  double scale, m02, m12;          // M = [[scale, 0, m02], [0, scale, m12], [0, 0, 1]]
  float far, near, comz, halfz;    // normalize_depth's float32 scalars
  float center[3];                 // image_to_3d(com)
};

// From the integer bounds on: resize size, letterbox offsets, nearest-neighbour steps and M (double), shared by prep_geom and prep_geom_f32
__host__ __device__ inline void prep_geom_layout(PrepGeom& g, int S) {
  const int wb = g.xe - g.xs, hb = g.ye - g.ys;
  if (wb <= 0 || hb <= 0) {  // a cube that projects to nothing (not reachable with positive focal lengths and cube sizes): an empty crop
    g.szw = g.szh = 0;
  } else if (wb > hb) {
    g.szw = S;
    g.szh = (int)((double)((long long)hb * S) / (double)wb);
  } else {
    g.szw = (int)((double)((long long)wb * S) / (double)hb);
    g.szh = S;
  }
  g.scale = hb > wb ? (double)g.szh / (double)hb : (double)g.szw / (double)(wb > 0 ? wb : 1);
  g.stepx = g.szw > 0 ? (double)wb / (double)g.szw : 0.0;
  g.stepy = g.szh > 0 ? (double)hb / (double)g.szh : 0.0;
  g.offx = (int)floor((double)S / 2.0 - (double)g.szw / 2.0);
  g.offy = (int)floor((double)S / 2.0 - (double)g.szh / 2.0);
  g.m02 = g.scale * (double)(-g.xs) + (double)g.offx;  // off . (scale . trans): one product, one sum, each rounded
  g.m12 = g.scale * (double)(-g.ys) + (double)g.offy;
}

// count / sums over the valid depth of the box (indices relative to the clipped box) -> everything crop_image and normalize_depth need
__host__ __device__ inline void prep_geom(unsigned long long cnt, unsigned long long sumx, unsigned long long sumy, unsigned long long sumd, const PrepBox& bx,
                                          const double* bbox, const double* cam, const double* cube, int S, PrepGeom& g) {
  double c0 = 0.0, c1 = 0.0, c2 = 300.0;
  if (cnt > 0) {
    // np.meshgrid(np.linspace(0, w, w), np.linspace(0, h, h)): sample i sits at i * (w / (w - 1)); the mean of the selected ones is the integer mean
    // times that step (the host sums the float64 coordinates pairwise: a few 1e-13 relative apart)
    const int w = bx.x1 - bx.x0, h = bx.y1 - bx.y0;
    const double sx = w > 1 ? (double)w / (double)(w - 1) : 0.0, sy = h > 1 ? (double)h / (double)(h - 1) : 0.0;
    c0 = (double)sumx * sx / (double)cnt;
    c1 = (double)sumy * sy / (double)cnt;
    c2 = (double)sumd / (double)cnt;  // exact integer sum, one division: the host's float64 mean of uint16 values bit for bit
    if (c2 <= 0) c2 = 300.0;
  }
  c0 += bbox[0];
  c1 += bbox[1];
  g.com[0] = c0;
  g.com[1] = c1;
  g.com[2] = c2;
  const double fx = cam[0], fy = cam[1], fu = cam[2], fv = cam[3];
  g.zs = c2 - cube[2] / 2.0;
  g.ze = c2 + cube[2] / 2.0;
  g.xs = (int)floor((c0 * c2 / fx - cube[0] / 2.0) / c2 * fx + 0.5);
  g.xe = (int)floor((c0 * c2 / fx + cube[0] / 2.0) / c2 * fx + 0.5);
  g.ys = (int)floor((c1 * c2 / fy - cube[1] / 2.0) / c2 * fy + 0.5);
  g.ye = (int)floor((c1 * c2 / fy + cube[1] / 2.0) / c2 * fy + 0.5);
  prep_geom_layout(g, S);
  g.far = (float)(c2 + cube[2] / 2.0);
  g.near = (float)(c2 - cube[2] / 2.0);
  g.comz = (float)c2;
  g.halfz = (float)(cube[2] / 2.0);
  g.center[0] = (float)((c0 - fu) * c2 / fx);
  g.center[1] = (float)((c1 - fv) * c2 / fy);
  g.center[2] = (float)c2;
}

// IEEE float32 division on either side (the device's default `/` may be the approximate one)
__host__ __device__ inline float prep_fdiv(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// a float bound as an integer; beyond +-2^28 (or NaN -> 0: a centre at depth 0, not a hand) it saturates, so that no later integer arithmetic overflows
__host__ __device__ inline int prep_bound_f32(float v) {
  const float f = floorf(v);
  return f >= 268435456.0f ? 268435456 : f <= -268435456.0f ? -268435456 : f == f ? (int)f : 0;
}

// preprocess.annotated_bounds + the scalars of normalize_depth and the round trip of the centre, for prepare_annotated: the centre cuvd (u, v, d mm) and the
// intrinsics are float32 and every operation up to the integer bounds is a float32 one in the reference's order (dataloader/loader.py:291-301 called with
// np.float32 operands); from the bounds on as prep_geom
__host__ __device__ inline void prep_geom_f32(const float* cuvd, const float* cam, const double* cube, int S, PrepGeom& g) {
  const float u = cuvd[0], v = cuvd[1], d = cuvd[2], fx = cam[0], fy = cam[1], fu = cam[2], fv = cam[3];
  const float hx = (float)(cube[0] / 2.0), hy = (float)(cube[1] / 2.0), hz = (float)(cube[2] / 2.0);
  g.com[0] = (double)u;
  g.com[1] = (double)v;
  g.com[2] = (double)d;
  const float zs = d - hz, ze = d + hz;
  g.zs = (double)zs;
  g.ze = (double)ze;
  g.xs = prep_bound_f32(prep_fdiv(prep_fdiv(u * d, fx) - hx, d) * fx + 0.5f);
  g.xe = prep_bound_f32(prep_fdiv(prep_fdiv(u * d, fx) + hx, d) * fx + 0.5f);
  g.ys = prep_bound_f32(prep_fdiv(prep_fdiv(v * d, fy) - hy, d) * fy + 0.5f);
  g.ye = prep_bound_f32(prep_fdiv(prep_fdiv(v * d, fy) + hy, d) * fy + 0.5f);
  prep_geom_layout(g, S);
  g.far = ze;
  g.near = zs;
  g.comz = d;
  g.halfz = hz;
  g.center[0] = prep_fdiv((u - fu) * d, fx);
  g.center[1] = prep_fdiv((v - fv) * d, fy);
  g.center[2] = d;
}

// Frame pixel behind crop pixel (oy, ox): false = letterbox border
__host__ __device__ inline bool prep_source(const PrepGeom& g, int oy, int ox, int& fy, int& fx) {
  const int ry = oy - g.offy, rx = ox - g.offx;
  if (ry < 0 || ry >= g.szh || rx < 0 || rx >= g.szw) return false;
  const int hb = g.ye - g.ys, wb = g.xe - g.xs;
  fy = g.ys + min((int)floor((double)ry * g.stepy), hb - 1);  // resize_nearest's index rule
  fx = g.xs + min((int)floor((double)rx * g.stepx), wb - 1);
  return true;
}

// get_crop's z-clamp on the sensor's uint16 values: nearer than the cube -> the near plane TRUNCATED to uint16, farther -> 0
__host__ __device__ inline unsigned short prep_zclamp(unsigned short v, const PrepGeom& g) {
  if (v != 0 && (double)v < g.zs) return (unsigned short)g.zs;
  if (v != 0 && (double)v > g.ze) return 0;
  return v;
}

// normalize_depth / normalize_img on one pixel (premax: the maximum of the z-clamped S x S crop), float32 like the host
__host__ __device__ inline float prep_normalize_f32(float v, float premax, float far, float near, float comz, float halfz) {
  if (v == premax) v = far;
  if (v == 0.0f) v = far;
  if (v >= far) v = far;
  if (v <= near) v = near;
  return prep_fdiv(v - comz, halfz);
}
// ... on the sensor's uint16 values, which float holds exactly
__host__ __device__ inline float prep_normalize(unsigned short raw, unsigned short premax, const PrepGeom& g) {
  return prep_normalize_f32((float)raw, (float)premax, g.far, g.near, g.comz, g.halfz);
}

// The tail of the dataset protocol's labels: the label normalised by the half cube (l0, l1, l2; double from here on: the reference's cube is an integer or
// float64 array) -> the point -> its projection, stored as float -> transformPoints2D with M = (scale, m02, m12) -> joint_img.  hx: cube[0] / 2; ctr: the
// float centre
__host__ __device__ inline void prep_label_to_image(double l0, double l1, double l2, double hx, const float* ctr, float fx, float fy, float fu, float fv,
                                                    double scale, double m02, double m12, int S, float* joint_img) {
  const double px = l0 * hx + (double)ctr[0], py = l1 * hx + (double)ctr[1], pz = l2 * hx + (double)ctr[2];  // curLabel * (cube[0] / 2.0) + com3D
  const float u = (float)(px * (double)fx / pz + (double)fu), v = (float)(py * (double)fy / pz + (double)fv), d = (float)pz;
  const float cu = (float)(scale * (double)u + m02), cv = (float)(scale * (double)v + m12);  // transformPoints2D, stored as float
  const float half = (float)((double)S / 2.0);
  joint_img[0] = prep_fdiv(cu, half) - 1.0f;
  joint_img[1] = prep_fdiv(cv, half) - 1.0f;
  joint_img[2] = (float)((double)(d - ctr[2]) / hx);
}

// ---- preprocess.depth_to_pcl for one pixel of the normalised crop: false = background; else the cube-normalised point clipped to [-1, 1]
struct PclGeom {
  double scale, m02, m12, fx, fy, fu, fv, cx, cy, cz, hx, hy, hz, cube2;
};
__host__ __device__ inline bool prep_point(float a, int row, int col, const PclGeom& g, float* out) {
  const bool mask = fabs((double)a - 1.0) <= (1e-8 + 1e-5 * 1.0) || a == 1.0f;  // np.isclose(img, 1)
  double dpt = (double)a * g.cube2 / 2.0 + g.cz;
  if (mask) dpt = 0.0;
  if (fabs(dpt) <= 1e-8) return false;  // np.isclose(dpt, 0)
  const double px = ((double)col + 0.5 - g.m02) / g.scale, py = ((double)row + 0.5 - g.m12) / g.scale;  // M^-1 (pixel centre)
  const double x = (px - g.fu) / g.fx * dpt, y = (py - g.fv) / g.fy * dpt;
  const double nx = (x - g.cx) / g.hx, ny = (y - g.cy) / g.hy, nz = (dpt - g.cz) / g.hz;
  out[0] = (float)fmin(fmax(nx, -1.0), 1.0);
  out[1] = (float)fmin(fmax(ny, -1.0), 1.0);
  out[2] = (float)fmin(fmax(nz, -1.0), 1.0);
  return true;
}

// ---- sampling keys: 36 hash bits | 14 bits candidate | 14 bits pixel.  Distinct ids give distinct elements, so the sorted order is one total order whatever
// network sorts it; the payload rides in the low bits.
__host__ __device__ inline unsigned prep_seed_base(long long seed) {
  return hash32((unsigned)(unsigned long long)seed ^ hash32((unsigned)((unsigned long long)seed >> 32) + 0x9e3779b9U));
}
__host__ __device__ inline unsigned long long prep_key(unsigned base, unsigned id, unsigned salt, unsigned cand, unsigned pix) {
  const unsigned h1 = hash32(base ^ hash32(id * 0x85ebca6bU + salt));
  const unsigned h2 = hash32(h1 + 0x68bc21ebU + id);
  return ((unsigned long long)h1 << 32) | ((unsigned long long)(h2 & 15u) << 28) | (unsigned long long)(cand << 14) | (unsigned long long)pix;
}

// ---- kpf_prep_augment_u16: everything one lane decides about a sample's augmentation (aug_geometry)
struct AugGeom {
  int warp;            // the RGB crop's warp: 0 none, 1 perspective (Ai), 2 affine (Ai[0..5] = i00 i01 i02 i10 i11 i12)
  int warp_depth;      // the depth crop's: the same, or 0 for an all-zero crop
  int zthresh;         // recropHand's z-threshold follows the depth warp
  int lab;             // labels: 0 unchanged, 1 shifted by the centre's move, 2 rotated in the image plane
  int has_color, status;
  float zs, ze;                          // the z-threshold's planes
  float far, near, comz, halfz, premax;  // normalize_img's float scalars (of the NEW centre and cube) and the pre-augmentation maximum
  float c3old[3], center[3], comu, comv; // back-projected old / final centre; the old centre in the image
  double Ai[9], c, s;
  double hx, hz;                         // new_cube[0] / 2, new_cube[2] / 2
  double scale, m02, m12;                // Mnew
  double color[3];
};

// ---- the LDS plan of a crop kernel, read by the kernel and by its launcher: a front slot at 0 (prep_crop_kernel: the box reduction's [4][PREP_NW] 64-bit
// sums; the dataset kernels: float xyz of up to 64 joints + the centre they are normalised by), the PrepGeom, the AugGeom (prep_augment_kernel), the
// [PREP_NW] wave maxima and the z-clamped crop [S * S] uint16.  Every slot but the last two is a 16-byte multiple.
constexpr int ANNOT_XYZ = 65 * 3;
constexpr int ANNOT_XYZ_BYTES = 800, PREP_GEOM_BYTES = 256, AUG_GEOM_BYTES = 320;
struct PrepLds {
  int geom, aug, wmax, crop;  // byte offsets
  constexpr size_t bytes(int S) const { return (size_t)crop + (size_t)S * S * 2; }
};
constexpr PrepLds prep_lds(int front, int aug) { return {front, front + PREP_GEOM_BYTES, front + PREP_GEOM_BYTES + aug, front + PREP_GEOM_BYTES + aug + PREP_NW * 4}; }
constexpr PrepLds PREP_LDS_CROP = prep_lds(4 * PREP_NW * 8, 0), PREP_LDS_ANNOT = prep_lds(ANNOT_XYZ_BYTES, 0), PREP_LDS_AUGMENT = prep_lds(ANNOT_XYZ_BYTES, AUG_GEOM_BYTES);
static_assert(sizeof(PrepGeom) <= PREP_GEOM_BYTES && PREP_GEOM_BYTES % 16 == 0, "PrepGeom outgrew its LDS slot");
static_assert(ANNOT_XYZ * 4 <= ANNOT_XYZ_BYTES && ANNOT_XYZ_BYTES % 16 == 0, "the joints outgrew their LDS slot");
static_assert(sizeof(AugGeom) <= AUG_GEOM_BYTES && AUG_GEOM_BYTES % 16 == 0, "AugGeom outgrew its LDS slot");

#ifdef __HIPCC__
// tuning aid: wall-clock stamps (100 MHz) of every workgroup's thread 0 at phase boundaries, [B][8] slots set by kpf_prep_set_stamps (NULL = off, the default):
// crop 0 start, 1 geometry published, 2 gather done, 3 end; sample 4 start, 5 candidates compacted and keyed, 6 sorted, 7 end
__device__ unsigned long long* kpf_prep_stamps = nullptr;
#define PREP_STAMP(i)                                                                                     \
  do {                                                                                                    \
    if (kpf_prep_stamps && threadIdx.x == 0) kpf_prep_stamps[8 * blockIdx.x + (i)] = wall_clock64();      \
  } while (0)

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Stored frame of sample b: b itself, or frame_index[b] of F (several tracks on one frame), clamped so that no index reads out of bounds
struct PrepFrame {
  const unsigned short* dep;
  const unsigned char* col;
};
__device__ __forceinline__ PrepFrame prep_frame(int b, const int* frame_index, int F, int Hs, int Ws, const unsigned short* depth, const unsigned char* rgb) {
  const int f = frame_index ? min(max(frame_index[b], 0), F - 1) : b;
  return {depth + (size_t)f * Hs * Ws, rgb + (size_t)f * Hs * Ws * 3};
}

// One lane: the per-sample small outputs of a crop kernel.  ctr / com3 / cube3 and M = (scale, m02, m12) are the sample's FINAL ones (the augmented ones
// in prep_augment_kernel), the bounds g's (the base crop's); the intrinsics come as double values, which hold a float exactly (cam_out is their rounding to
// float: the value itself where they were floats).  cam64 / cube64 may be NULL.
__device__ __forceinline__ void prep_publish(int b, const PrepGeom& g, const float* ctr, const double* com3, const double* cube3, double fx, double fy, double fu,
                                             double fv, double scale, double m02, double m12, float* center, double* com, float* cube_out, float* cam_out,
                                             double* cam64, double* cube64, float* M, double* Md, int* bounds) {
  for (int k = 0; k < 3; ++k) {
    center[3 * b + k] = ctr[k];
    com[3 * b + k] = com3[k];
    cube_out[3 * b + k] = (float)cube3[k];
    if (cube64) cube64[3 * b + k] = cube3[k];
  }
  const double c[4] = {fx, fy, fu, fv};
  for (int k = 0; k < 4; ++k) {
    cam_out[4 * b + k] = (float)c[k];
    if (cam64) cam64[4 * b + k] = c[k];
  }
  const double m[9] = {scale, 0.0, m02, 0.0, scale, m12, 0.0, 0.0, 1.0};
  for (int k = 0; k < 9; ++k) {
    Md[9 * b + k] = m[k];
    M[9 * b + k] = (float)m[k];
  }
  const int bo[6] = {g.xs, g.xe, g.ys, g.ye, g.szw, g.szh};
  for (int k = 0; k < 6; ++k) bounds[6 * b + k] = bo[k];
}

// Offset, in the stored window, of the frame pixel behind crop pixel (oyp, oxp): false = letterbox border, outside the frame or outside the window (all read
// as 0).  A mirrored sample's logical pixel (fy, fx) of the H x W frame is TRUE column W - 1 - fx, and the stored window is tested against that true column.
__device__ __forceinline__ bool prep_window_offset(const PrepGeom& g, int oyp, int oxp, int mirror, int Hs, int Ws, int ox, int oy, int H, int W, size_t& s) {
  int fy, fx;
  if (!(prep_source(g, oyp, oxp, fy, fx) && fy >= 0 && fy < H && fx >= 0 && fx < W)) return false;
  const int wy = fy - oy, wx = (mirror ? W - 1 - fx : fx) - ox;
  if (!(wy >= 0 && wy < Hs && wx >= 0 && wx < Ws)) return false;
  s = (size_t)wy * Ws + wx;
  return true;
}

// Phase 3 of a crop, shared by prep_crop_kernel (mirror = 0), prep_annot_kernel and prep_augment_kernel (img_rgb NULL: its RGB goes through the warp): the
// z-clamped depth crop into LDS and RGB straight out; returns the maximum of the crop, which decides the far plane.  All PREP_NT threads of the workgroup;
// contains a barrier, after which crop[] is complete.
__device__ __forceinline__ unsigned prep_gather(const PrepGeom& g, const unsigned short* __restrict__ dep, const unsigned char* __restrict__ col, int mirror, int Hs,
                                                int Ws, int ox, int oy, int H, int W, int S, unsigned short* crop, unsigned* wmax, float* __restrict__ img_rgb) {
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int P = S * S;
  unsigned mx = 0;
  for (int p = t; p < P; p += PREP_NT) {
    const int oyp = p / S, oxp = p - oyp * S;
    size_t s;
    unsigned short v = 0;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (prep_window_offset(g, oyp, oxp, mirror, Hs, Ws, ox, oy, H, W, s)) {
      v = prep_zclamp(dep[s], g);
      if (img_rgb) {
        c0 = (float)col[3 * s];
        c1 = (float)col[3 * s + 1];
        c2 = (float)col[3 * s + 2];
      }
    }
    crop[p] = v;
    mx = max(mx, (unsigned)v);
    if (img_rgb) {
      float* o = img_rgb + (size_t)b * 3 * P + p;
      o[0] = __fdiv_rn(c0, 255.0f);
      o[P] = __fdiv_rn(c1, 255.0f);
      o[2 * (size_t)P] = __fdiv_rn(c2, 255.0f);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
  if (lane == 0) wmax[wv] = mx;
  __syncthreads();
  PREP_STAMP(2);
  unsigned premax = 0;
  for (int w = 0; w < PREP_NW; ++w) premax = max(premax, wmax[w]);
  return premax;
}

// Phases 3 and 4 of a crop: prep_gather, then normalize_depth.
__device__ __forceinline__ void prep_gather_normalize(const PrepGeom& g, const unsigned short* __restrict__ dep, const unsigned char* __restrict__ col, int mirror,
                                                      int Hs, int Ws, int ox, int oy, int H, int W, int S, unsigned short* crop, unsigned* wmax,
                                                      float* __restrict__ img, float* __restrict__ img_rgb) {
  const int b = blockIdx.x, t = threadIdx.x, P = S * S;
  const unsigned premax = prep_gather(g, dep, col, mirror, Hs, Ws, ox, oy, H, W, S, crop, wmax, img_rgb);
  for (int p = t; p < P; p += PREP_NT) img[(size_t)b * P + p] = prep_normalize(crop[p], (unsigned short)premax, g);
}

__global__ __launch_bounds__(PREP_NT) void prep_crop_kernel(const unsigned char* __restrict__ rgb, const unsigned short* __restrict__ depth,
                                                            const int* __restrict__ frame_index, int F, const double* __restrict__ bbox, const double* __restrict__ cam, const double* __restrict__ cube,
                                                            int Hs, int Ws, int ox, int oy, int H, int W, int S, float* __restrict__ img,
                                                            float* __restrict__ img_rgb, float* __restrict__ center, float* __restrict__ M,
                                                            float* __restrict__ cube_out, float* __restrict__ cam_out, double* __restrict__ com,
                                                            int* __restrict__ bounds, double* __restrict__ Md) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* red = reinterpret_cast<unsigned long long*>(smem);  // [4][PREP_NW]
  PrepGeom* gs = reinterpret_cast<PrepGeom*>(smem + PREP_LDS_CROP.geom);
  unsigned* wmax = reinterpret_cast<unsigned*>(smem + PREP_LDS_CROP.wmax);
  unsigned short* crop = reinterpret_cast<unsigned short*>(smem + PREP_LDS_CROP.crop);
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const PrepFrame fr = prep_frame(b, frame_index, F, Hs, Ws, depth, rgb);
  const unsigned short* dep = fr.dep;
  const double* bb = bbox + 4 * b;

  // 1. centre of mass over the box: pixels outside the stored window read as 0, which is invalid depth, so only the intersection is visited
  PREP_STAMP(0);
  const PrepBox bx = prep_box(bb, H, W);
  const int wx0 = max(bx.x0, ox), wx1 = min(bx.x1, ox + Ws), wy0 = max(bx.y0, oy), wy1 = min(bx.y1, oy + Hs);
  const int bw = max(wx1 - wx0, 0), bh = max(wy1 - wy0, 0);
  unsigned long long cnt = 0, sx = 0, sy = 0, sd = 0;
  for (int y = wy0 + wv; y < wy0 + bh; y += PREP_NW)  // one wave per row: coalesced 128-byte reads
    for (int x = wx0 + lane; x < wx0 + bw; x += 64) {
      const unsigned v = dep[(size_t)(y - oy) * Ws + (x - ox)];
      if (v >= 171u && v <= 1500u) {
        cnt += 1;
        sx += (unsigned)(x - bx.x0);
        sy += (unsigned)(y - bx.y0);
        sd += v;
      }
    }
  cnt = wave_sum_u64(cnt);
  sx = wave_sum_u64(sx);
  sy = wave_sum_u64(sy);
  sd = wave_sum_u64(sd);
  if (lane == 0) {
    red[0 * PREP_NW + wv] = cnt;
    red[1 * PREP_NW + wv] = sx;
    red[2 * PREP_NW + wv] = sy;
    red[3 * PREP_NW + wv] = sd;
  }
  __syncthreads();
  // 2. one lane finishes in double and publishes the geometry
  if (t == 0) {
    unsigned long long a[4] = {0, 0, 0, 0};
    for (int q = 0; q < 4; ++q)
      for (int w = 0; w < PREP_NW; ++w) a[q] += red[q * PREP_NW + w];
    PrepGeom g;
    const double* cm = cam + 4 * b;
    prep_geom(a[0], a[1], a[2], a[3], bx, bb, cm, cube + 3 * b, S, g);
    *gs = g;
    prep_publish(b, g, g.center, g.com, cube + 3 * b, cm[0], cm[1], cm[2], cm[3], g.scale, g.m02, g.m12, center, com, cube_out, cam_out, nullptr, nullptr, M, Md,
                 bounds);
  }
  __syncthreads();
  const PrepGeom g = *gs;
  PREP_STAMP(1);
  // 3. gather, 4. normalize_depth
  prep_gather_normalize(g, dep, fr.col, 0, Hs, Ws, ox, oy, H, W, S, crop, wmax, img, img_rgb);
  PREP_STAMP(3);
}

// kpf_prep_annot_u16: the crop by the dataset protocol (preprocess.prepare_annotated).  Phase 0 replaces the box reduction: the centre comes from the annotation.

// Phase 0a of the dataset protocol, one lane per joint: the joint's xyz in float.  through_image: DexYCB's item takes the joints through the image and back,
// mirrored or not; HO3D's item (the one with a given centre) uses them as they are
__device__ __forceinline__ void annot_joint_xyz(const float* jp, const float* cam, bool through_image, int mir, int W, float* out) {
  const float fx = cam[0], fy = cam[1], fu = cam[2], fv = cam[3];
  float x = jp[0], y = jp[1];
  const float z = jp[2];
  if (through_image) {
    float u = prep_fdiv(x * fx, z) + fu;
    const float v = prep_fdiv(y * fy, z) + fv;
    if (mir) u = ((float)W - u) - 1.0f;
    x = prep_fdiv((u - fu) * z, fx);
    y = prep_fdiv((v - fv) * z, fy);
  }
  out[0] = x;
  out[1] = y;
  out[2] = z;
}

// Phase 0b, one lane: the centre (given, or the rows of xyz summed in order: np.mean(0) of a [J][3] float array) into xyz[64], its projection, the geometry
__device__ __forceinline__ void annot_centre_geom(float* xyz, const float* given, int J, const float* cam, const double* cube, int S, PrepGeom& g) {
  const float fx = cam[0], fy = cam[1], fu = cam[2], fv = cam[3];
  float c[3] = {0.f, 0.f, 0.f};
  if (given) {
    for (int k = 0; k < 3; ++k) c[k] = given[k];
  } else {
    for (int j = 0; j < J; ++j)
      for (int k = 0; k < 3; ++k) c[k] = c[k] + xyz[3 * j + k];
    for (int k = 0; k < 3; ++k) c[k] = prep_fdiv(c[k], (float)J);
  }
  for (int k = 0; k < 3; ++k) xyz[3 * 64 + k] = c[k];
  const float cuvd[3] = {prep_fdiv(c[0] * fx, c[2]) + fu, prep_fdiv(c[1] * fy, c[2]) + fv, c[2]};
  prep_geom_f32(cuvd, cam, cube, S, g);
}
__global__ __launch_bounds__(PREP_NT) void prep_annot_kernel(const unsigned char* __restrict__ rgb, const unsigned short* __restrict__ depth,
                                                             const int* __restrict__ frame_index, int F, const float* __restrict__ joints,
                                                             const float* __restrict__ cam, const float* __restrict__ center_xyz,
                                                             const unsigned char* __restrict__ mirror, const double* __restrict__ cube, int J, int Hs, int Ws,
                                                             int ox, int oy, int H, int W, int S, float* __restrict__ img, float* __restrict__ img_rgb,
                                                             float* __restrict__ center, float* __restrict__ M, float* __restrict__ cube_out,
                                                             float* __restrict__ cam_out, double* __restrict__ com, int* __restrict__ bounds,
                                                             double* __restrict__ Md, float* __restrict__ joint, float* __restrict__ joint_img,
                                                             double* __restrict__ cam64) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xyz = reinterpret_cast<float*>(smem);  // [65][3]
  PrepGeom* gs = reinterpret_cast<PrepGeom*>(smem + PREP_LDS_ANNOT.geom);
  unsigned* wmax = reinterpret_cast<unsigned*>(smem + PREP_LDS_ANNOT.wmax);
  unsigned short* crop = reinterpret_cast<unsigned short*>(smem + PREP_LDS_ANNOT.crop);
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const PrepFrame fr = prep_frame(b, frame_index, F, Hs, Ws, depth, rgb);
  const int mir = mirror[b] ? 1 : 0;
  const float fx = cam[4 * b], fy = cam[4 * b + 1], fu = cam[4 * b + 2], fv = cam[4 * b + 3];
  PREP_STAMP(0);
  // 0a. one lane per joint: uvd, the mirror and xyz in float.  DexYCB's item takes the joints through the image and back, mirrored or not; HO3D's item (the
  // one with a given centre) uses them as they are
  if (wv == 0 && joints && lane < J) annot_joint_xyz(joints + ((size_t)b * J + lane) * 3, cam + 4 * b, !center_xyz || mir, mir, W, xyz + 3 * lane);
  __syncthreads();
  // 0b. one lane: the centre (given, or the rows summed in order: np.mean(0) of a [J][3] float array), its projection, the geometry
  if (t == 0) {
    PrepGeom g;
    annot_centre_geom(xyz, center_xyz ? center_xyz + 3 * b : nullptr, J, cam + 4 * b, cube + 3 * b, S, g);
    *gs = g;
    prep_publish(b, g, g.center, g.com, cube + 3 * b, fx, fy, fu, fv, g.scale, g.m02, g.m12, center, com, cube_out, cam_out, cam64, nullptr, M, Md, bounds);
  }
  __syncthreads();
  const PrepGeom g = *gs;
  PREP_STAMP(1);
  // 0c. the labels, one lane per joint: float up to the division by the half cube (a float32 division here), double from there
  if (wv == 0 && lane < J) {
    float lab[3] = {0.f, 0.f, 0.f}, uvd[3] = {0.f, 0.f, 0.f};
    if (joints) {
      for (int k = 0; k < 3; ++k) lab[k] = prep_fdiv(xyz[3 * lane + k] - xyz[3 * 64 + k], g.halfz);
      prep_label_to_image((double)lab[0], (double)lab[1], (double)lab[2], cube[3 * b] / 2.0, g.center, fx, fy, fu, fv, g.scale, g.m02, g.m12, S, uvd);
    }
    for (int k = 0; k < 3; ++k) {
      joint[((size_t)b * J + lane) * 3 + k] = lab[k];
      joint_img[((size_t)b * J + lane) * 3 + k] = uvd[k];
    }
  }
  // 3. gather, 4. normalize_depth
  prep_gather_normalize(g, fr.dep, fr.col, mir, Hs, Ws, ox, oy, H, W, S, crop, wmax, img, img_rgb);
  PREP_STAMP(3);
}

// ---- kpf_prep_augment_u16: the training item (preprocess.prepare_augmented)
__host__ __device__ inline bool aug_finite(double v) { return v - v == 0.0; }

// loader.comToTransform for centre cuvd and cube `size`: the bounds in float (prep_geom_f32), the letterbox offset from the UNTRUNCATED resize size
__host__ __device__ inline bool aug_transform(const float* cuvd, const float* cam, const double* size, int S, double& scale, double& m02, double& m12) {
  PrepGeom q;
  prep_geom_f32(cuvd, cam, size, S, q);
  const int wb = q.xe - q.xs, hb = q.ye - q.ys;
  const int sat = 268435456;  // prep_bound_f32's saturation: a bound that reached it is not a bound (the host refuses it too)
  if (wb <= 0 || hb <= 0 || abs(q.xs) >= sat || abs(q.xe) >= sat || abs(q.ys) >= sat || abs(q.ye) >= sat) return false;
  double sz0, sz1;
  if (wb > hb) {
    scale = (double)S / (double)wb;
    sz0 = (double)S;
    sz1 = (double)hb * (double)S / (double)wb;
  } else {
    scale = (double)S / (double)hb;
    sz0 = (double)wb * (double)S / (double)hb;
    sz1 = (double)S;
  }
  const double x0 = floor((double)S / 2.0 - sz0 / 2.0), y0 = floor((double)S / 2.0 - sz1 / 2.0);
  m02 = scale * (double)(-q.xs) + x0;
  m12 = scale * (double)(-q.ys) + y0;
  return true;
}

// One lane: the augmented geometry in the host's precisions and operation order (prepare_augmented).  g: the base crop's geometry; premax: its maximum.
__host__ __device__ inline void aug_geometry(const PrepGeom& g, const float* cam, const double* cube, int mode, const double* off, double sc, double rot,
                                             const double* rot_cs, const double* color, unsigned premax, int S, AugGeom& a, double* cube_new, float* com_new) {
  const float cuvd[3] = {(float)g.com[0], (float)g.com[1], (float)g.com[2]};  // (exact: g.com holds floats)
  const double c = rot_cs[0], s = rot_cs[1];
  bool finite = aug_finite(off[0]) && aug_finite(off[1]) && aug_finite(off[2]) && aug_finite(rot) && aug_finite(sc) && aug_finite(c) && aug_finite(s) && sc > 0.0;
  if (color) finite = finite && aug_finite(color[0]) && aug_finite(color[1]) && aug_finite(color[2]);
  double ncube[3] = {cube[0], cube[1], cube[2]};
  float ncom[3] = {cuvd[0], cuvd[1], cuvd[2]};
  double scale = g.scale, m02 = g.m02, m12 = g.m12;
  int warp = 0, lab = 0;
  bool moved = false, ok = finite, scaled = false;
  if (finite && mode == 1 && !(fabs(off[0]) <= 1e-8 && fabs(off[1]) <= 1e-8 && fabs(off[2]) <= 1e-8)) {
    const double p0 = (double)g.center[0] + off[0], p1 = (double)g.center[1] + off[1], p2 = (double)g.center[2] + off[2];
    ncom[0] = (float)(p0 * (double)cam[0] / p2 + (double)cam[2]);
    ncom[1] = (float)(p1 * (double)cam[1] / p2 + (double)cam[3]);
    ncom[2] = (float)p2;
    lab = 1;
    if (!(aug_finite((double)ncom[0]) && aug_finite((double)ncom[1]) && aug_finite((double)ncom[2]))) {
      ok = false;  // the offset moved the centre into the camera plane: refused
    } else if (!(fabs((double)cuvd[2]) <= 1e-8 || fabs((double)ncom[2]) <= 1e-8)) {
      moved = true;
      ok = aug_transform(ncom, cam, cube, S, scale, m02, m12);
    }
  } else if (finite && mode == 2 && !(fabs(sc - 1.0) <= 1e-8 + 1e-5 * fabs(1.0))) {
    for (int k = 0; k < 3; ++k) ncube[k] = cube[k] * sc;
    scaled = true;
    if (!(fabs((double)cuvd[2]) <= 1e-8)) {
      moved = true;
      ok = aug_transform(cuvd, cam, ncube, S, scale, m02, m12);
    }
  } else if (finite && mode == 0 && !(fabs(rot) <= 1e-8)) {
    warp = 2;
    lab = 2;
  }
  if (ok && moved) {
    // A = np.dot(Mnew, np.linalg.inv(M)) on crop matrices: inv = [[1/s, 0, (-t)(1/s)], ...], every product and the one sum rounded separately
    const double r = 1.0 / g.scale, i02 = -g.m02 * r, i12 = -g.m12 * r;
    const double A[9] = {scale * r, 0.0, scale * i02 + m02, 0.0, scale * r, scale * i12 + m12, 0.0, 0.0, 1.0};
    bool fin = A[0] != 0.0 && A[4] != 0.0;
    for (int k = 0; k < 9; ++k) fin = fin && aug_finite(A[k]);
    if (!fin) {
      ok = false;
    } else {
      const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
      const double d = 1.0 / det;
      a.Ai[0] = (A[4] * A[8] - A[5] * A[7]) * d;
      a.Ai[1] = (A[2] * A[7] - A[1] * A[8]) * d;
      a.Ai[2] = (A[1] * A[5] - A[2] * A[4]) * d;
      a.Ai[3] = (A[5] * A[6] - A[3] * A[8]) * d;
      a.Ai[4] = (A[0] * A[8] - A[2] * A[6]) * d;
      a.Ai[5] = (A[2] * A[3] - A[0] * A[5]) * d;
      a.Ai[6] = (A[3] * A[7] - A[4] * A[6]) * d;
      a.Ai[7] = (A[1] * A[6] - A[0] * A[7]) * d;
      a.Ai[8] = (A[0] * A[4] - A[1] * A[3]) * d;
      warp = 1;
    }
  }
  a.status = 0;
  a.has_color = color ? 1 : 0;
  if (!ok) {  // refused: mode none, no colour
    a.status = 2;
    a.has_color = 0;
    warp = lab = 0;
    scaled = false;
    for (int k = 0; k < 3; ++k) {
      ncube[k] = cube[k];
      ncom[k] = cuvd[k];
    }
    scale = g.scale, m02 = g.m02, m12 = g.m12;
  }
  if (warp == 2) {
    // cv2.getRotationMatrix2D((S / 2, S / 2), -rot, 1) and warpAffine's closed-form inverse
    const double cx = (double)(S / 2), cy = cx, al = c, be = -s;
    const double m00 = al, m01 = be, m2 = (1.0 - al) * cx - be * cy, m10 = -be, m11 = al, m5 = be * cx + (1.0 - al) * cy;
    double D = m00 * m11 - m01 * m10;
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double i00 = m11 * D, i11 = m00 * D, i01 = m01 * -D, i10 = m10 * -D;
    a.Ai[0] = i00;
    a.Ai[1] = i01;
    a.Ai[2] = -i00 * m2 - i01 * m5;
    a.Ai[3] = i10;
    a.Ai[4] = i11;
    a.Ai[5] = -i10 * m2 - i11 * m5;
  }
  a.warp = warp;
  a.c = c;
  a.s = s;
  if (a.has_color)
    for (int k = 0; k < 3; ++k) a.color[k] = color[k];
  for (int k = 0; k < 3; ++k) a.c3old[k] = g.center[k];
  a.comu = cuvd[0];
  a.comv = cuvd[1];
  a.premax = (float)premax;
  if (premax == 0) {  // an all-zero depth crop: depth, labels, centre, M and cube stay (the RGB crop is warped all the same)
    a.warp_depth = a.zthresh = a.lab = 0;
    for (int k = 0; k < 3; ++k) {
      ncube[k] = cube[k];
      ncom[k] = cuvd[k];
    }
    scale = g.scale, m02 = g.m02, m12 = g.m12;
  } else {
    a.warp_depth = warp;
    a.zthresh = warp == 1;
    a.lab = lab;
    if (warp != 0 || lab != 0 || scaled) a.status |= 1;
  }
  // recropHand's z-threshold: the centre after the move with the OLD cube (also in mode sc); normalize_img: the new centre and the new cube, in float
  const float hzold = (float)(cube[2] / 2.0), hz = (float)(ncube[2] / 2.0);
  a.zs = ncom[2] - hzold;
  a.ze = ncom[2] + hzold;
  a.far = ncom[2] + hz;
  a.near = ncom[2] - hz;
  a.comz = ncom[2];
  a.halfz = hz;
  a.hx = ncube[0] / 2.0;
  a.hz = ncube[2] / 2.0;
  a.scale = scale;
  a.m02 = m02;
  a.m12 = m12;
  a.center[0] = prep_fdiv((ncom[0] - cam[2]) * ncom[2], cam[0]);
  a.center[1] = prep_fdiv((ncom[1] - cam[3]) * ncom[2], cam[1]);
  a.center[2] = ncom[2];
  for (int k = 0; k < 3; ++k) {
    cube_new[k] = ncube[k];
    com_new[k] = ncom[k];
  }
}

// Crop pixel behind destination pixel (y, x) of a warp (the rule of preprocess.warp_perspective_nearest / warp_affine_nearest): false = border.  No integer
// is formed from a value that is not finite or out of range.
__host__ __device__ inline bool aug_source(int warp, const double* Ai, int y, int x, int S, int& Y, int& X) {
  if (warp == 0) {
    Y = y;
    X = x;
    return true;
  }
  const double xd = (double)x, yd = (double)y;
  if (warp == 1) {
    double W = (Ai[6] * xd + Ai[7] * yd) + Ai[8];
    W = W != 0.0 ? 1.0 / W : 0.0;
    const double Xd = rint((Ai[0] * xd + (Ai[1] * yd + Ai[2])) * W), Yd = rint((Ai[3] * xd + (Ai[4] * yd + Ai[5])) * W);
    if (!(Xd >= 0.0 && Xd < (double)S && Yd >= 0.0 && Yd < (double)S)) return false;  // (NaN compares false)
    X = (int)Xd;
    Y = (int)Yd;
    return true;
  }
  const double tx0 = rint((Ai[1] * yd + Ai[2]) * 1024.0), tx1 = rint((Ai[0] * xd) * 1024.0);
  const double ty0 = rint((Ai[4] * yd + Ai[5]) * 1024.0), ty1 = rint((Ai[3] * xd) * 1024.0);
  const double lim = 1099511627776.0;  // 2^40
  if (!(fabs(tx0) < lim && fabs(tx1) < lim && fabs(ty0) < lim && fabs(ty1) < lim)) return false;
  const long long Xl = ((long long)tx0 + 512 + (long long)tx1) >> 10, Yl = ((long long)ty0 + 512 + (long long)ty1) >> 10;
  if (!(Xl >= 0 && Xl < S && Yl >= 0 && Yl < S)) return false;
  X = (int)Xl;
  Y = (int)Yl;
  return true;
}

// sampling-style counter hash for the augmentation draw: uniform i of a sample = 53 bits of words 2 i and 2 i + 1, times 2^-53
constexpr unsigned AUG_SALT = 0xa4093822U;
__host__ __device__ inline double aug_uniform(unsigned base, unsigned i) {
  const unsigned w0 = hash32(base ^ hash32((2u * i) * 0x85ebca6bU + AUG_SALT)), w1 = hash32(base ^ hash32((2u * i + 1u) * 0x85ebca6bU + AUG_SALT));
  return (double)(((unsigned long long)w0 << 21) | (unsigned long long)(w1 >> 11)) * 1.1102230246251565e-16;  // 2^-53
}

__global__ __launch_bounds__(PREP_NT) void prep_augment_kernel(const unsigned char* __restrict__ rgb, const unsigned short* __restrict__ depth,
                                                               const int* __restrict__ frame_index, int F, const float* __restrict__ joints,
                                                               const float* __restrict__ cam, const float* __restrict__ center_xyz,
                                                               const unsigned char* __restrict__ mirror, const double* __restrict__ cube,
                                                               const int* __restrict__ mode, const double* __restrict__ off, const double* __restrict__ sc,
                                                               const double* __restrict__ rot, const double* __restrict__ rot_cs, const double* __restrict__ color,
                                                               int J, int Hs, int Ws, int ox, int oy, int H, int W, int S, float* __restrict__ img,
                                                               float* __restrict__ img_rgb, float* __restrict__ center, float* __restrict__ M,
                                                               float* __restrict__ cube_out, float* __restrict__ cam_out, double* __restrict__ com,
                                                               int* __restrict__ bounds, double* __restrict__ Md, float* __restrict__ joint,
                                                               float* __restrict__ joint_img, double* __restrict__ cam64, double* __restrict__ cube64,
                                                               int* __restrict__ aug_status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xyz = reinterpret_cast<float*>(smem);  // [65][3]
  PrepGeom* gs = reinterpret_cast<PrepGeom*>(smem + PREP_LDS_AUGMENT.geom);
  AugGeom* as = reinterpret_cast<AugGeom*>(smem + PREP_LDS_AUGMENT.aug);
  unsigned* wmax = reinterpret_cast<unsigned*>(smem + PREP_LDS_AUGMENT.wmax);
  unsigned short* crop = reinterpret_cast<unsigned short*>(smem + PREP_LDS_AUGMENT.crop);
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, P = S * S;
  const PrepFrame fr = prep_frame(b, frame_index, F, Hs, Ws, depth, rgb);
  const unsigned char* col = fr.col;
  const int mir = mirror[b] ? 1 : 0;
  const float fx = cam[4 * b], fy = cam[4 * b + 1], fu = cam[4 * b + 2], fv = cam[4 * b + 3];
  PREP_STAMP(0);
  // 1. joints, centre and base geometry exactly as prep_annot_kernel
  if (wv == 0 && lane < J) annot_joint_xyz(joints + ((size_t)b * J + lane) * 3, cam + 4 * b, !center_xyz || mir, mir, W, xyz + 3 * lane);
  __syncthreads();
  if (t == 0) {
    PrepGeom g;
    annot_centre_geom(xyz, center_xyz ? center_xyz + 3 * b : nullptr, J, cam + 4 * b, cube + 3 * b, S, g);
    *gs = g;
  }
  __syncthreads();
  const PrepGeom g = *gs;
  PREP_STAMP(1);
  // 2. the z-clamped base depth crop into LDS and its maximum (RGB is read through the warp in phase 5)
  const unsigned premax = prep_gather(g, fr.dep, col, mir, Hs, Ws, ox, oy, H, W, S, crop, wmax, nullptr);
  // 3. one lane: the augmented geometry, and the sample's small outputs
  if (t == 0) {
    AugGeom a;
    double ncube[3];
    float ncom[3];
    aug_geometry(g, cam + 4 * b, cube + 3 * b, mode[b], off + 3 * b, sc[b], rot[b], rot_cs + 2 * b, color ? color + 3 * b : nullptr, premax, S, a, ncube, ncom);
    *as = a;
    const double ncom64[3] = {(double)ncom[0], (double)ncom[1], (double)ncom[2]};
    prep_publish(b, g, a.center, ncom64, ncube, fx, fy, fu, fv, a.scale, a.m02, a.m12, center, com, cube_out, cam_out, cam64, cube64, M, Md, bounds);
    aug_status[b] = a.status;
  }
  __syncthreads();
  // 4. the labels, one lane per joint: float up to the division by the half cube, double from there (the reference's cube is an integer or float64 array)
  if (wv == 0 && lane < J) {
    const int lab = as->lab;
    float l[3];
    for (int k = 0; k < 3; ++k) l[k] = xyz[3 * lane + k] - xyz[3 * 64 + k];
    const float cn[3] = {as->center[0], as->center[1], as->center[2]};
    if (lab == 1) {
      for (int k = 0; k < 3; ++k) l[k] = (l[k] + as->c3old[k]) - cn[k];
    } else if (lab == 2) {
      const float q0 = l[0] + as->c3old[0], q1 = l[1] + as->c3old[1], q2 = l[2] + as->c3old[2];
      const float u = prep_fdiv(q0 * fx, q2) + fu, v = prep_fdiv(q1 * fy, q2) + fv;
      const float pp0 = u - as->comu, pp1 = v - as->comv;
      const double c = as->c, s = as->s;
      float r0 = (float)((double)pp0 * c - (double)pp1 * s), r1 = (float)((double)pp0 * s + (double)pp1 * c);
      r0 = r0 + as->comu;
      r1 = r1 + as->comv;
      l[0] = prep_fdiv((r0 - fu) * q2, fx) - as->c3old[0];
      l[1] = prep_fdiv((r1 - fv) * q2, fy) - as->c3old[1];
      l[2] = q2 - as->c3old[2];
    }
    const double hx = as->hx, hz = as->hz;
    const double l0 = (double)l[0] / hz, l1 = (double)l[1] / hz, l2 = (double)l[2] / hz;
    float* jo = joint + ((size_t)b * J + lane) * 3;
    jo[0] = (float)l0;
    jo[1] = (float)l1;
    jo[2] = (float)l2;
    prep_label_to_image(l0, l1, l2, hx, cn, fx, fy, fu, fv, as->scale, as->m02, as->m12, S, joint_img + ((size_t)b * J + lane) * 3);
  }
  // 5. every destination pixel through the inverse map: depth from LDS (z-threshold, premax rule, normalisation in float), RGB from the frame
  const int warp = as->warp, warp_depth = as->warp_depth, zthresh = as->zthresh, has_color = as->has_color;
  const float zs = as->zs, ze = as->ze, far = as->far, near = as->near, comz = as->comz, halfz = as->halfz, pmx = as->premax;
  double Ai[9];
  for (int k = 0; k < 9; ++k) Ai[k] = as->Ai[k];
  double cs[3] = {1.0, 1.0, 1.0};
  if (has_color)
    for (int k = 0; k < 3; ++k) cs[k] = as->color[k];
  for (int p = t; p < P; p += PREP_NT) {
    const int y = p / S, x = p - y * S;
    int Y = 0, X = 0;
    const bool in = aug_source(warp, Ai, y, x, S, Y, X);
    float v = 0.f;
    if (warp_depth == 0)
      v = (float)crop[p];
    else if (in)
      v = (float)crop[Y * S + X];  // (0 <= Y, X < S: tested by aug_source)
    if (zthresh) {
      const bool m1 = v < zs && v != 0.f, m2 = v > ze && v != 0.f;
      if (m1) v = zs;
      if (m2) v = 0.f;
    }
    img[(size_t)b * P + p] = prep_normalize_f32(v, pmx, far, near, comz, halfz);
    float c3[3] = {0.f, 0.f, 0.f};
    size_t so;
    if (in && prep_window_offset(g, Y, X, mir, Hs, Ws, ox, oy, H, W, so))
      for (int k = 0; k < 3; ++k) c3[k] = (float)col[3 * so + k];
    if (has_color)
      for (int k = 0; k < 3; ++k) c3[k] = (float)fmin(fmax((double)c3[k] * cs[k], 0.0), 255.0);
    float* o = img_rgb + (size_t)b * 3 * P + p;
    o[0] = __fdiv_rn(c3[0], 255.0f);
    o[P] = __fdiv_rn(c3[1], 255.0f);
    o[2 * (size_t)P] = __fdiv_rn(c3[2], 255.0f);
  }
  PREP_STAMP(3);
}

// kpf_prep_aug_draw: one thread per sample (preprocess.draw_augment is the host twin)
__global__ __launch_bounds__(256) void prep_aug_draw_kernel(long long* __restrict__ seed, int B, double sigma_com, double sigma_sc, double rot_range, double cf,
                                                            long long stride, int* __restrict__ mode, double* __restrict__ off, double* __restrict__ sc,
                                                            double* __restrict__ rot, double* __restrict__ rot_cs, double* __restrict__ color) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const long long sd = seed[b];
  const unsigned base = prep_seed_base(sd);
  mode[b] = (int)floor(4.0 * aug_uniform(base, 0));
  for (int k = 0; k < 3; ++k) off[3 * b + k] = (-1.0 + 2.0 * aug_uniform(base, 1 + k)) * sigma_com;
  const double r = -rot_range + (rot_range - -rot_range) * aug_uniform(base, 4);
  rot[b] = r;
  sc[b] = fabs(1.0 + (-1.0 + 2.0 * aug_uniform(base, 5)) * sigma_sc);
  for (int k = 0; k < 3; ++k) color[3 * b + k] = (1.0 - cf) + ((1.0 + cf) - (1.0 - cf)) * aug_uniform(base, 6 + k);
  double m = fmod(r, 360.0);  // np.mod: the sign of the divisor
  if (m != 0.0 && m < 0.0) m += 360.0;
  const double al = m * 3.141592653589793 / 180.0;
  rot_cs[2 * b] = cos(al);
  rot_cs[2 * b + 1] = sin(al);
  seed[b] = sd + stride;
}
// Sorts a[0, P2) ascending (P2 a power of two), all PREP_NT threads of the workgroup; ends with a barrier.
__device__ __forceinline__ void prep_bitonic_sort(unsigned long long* a, int P2) {
  const int t = threadIdx.x;
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (P2 >> 1); p += PREP_NT) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), x = i | j;
        const unsigned long long u = a[i], v = a[x];
        if ((u > v) == ((i & k) == 0)) {
          a[i] = v;
          a[x] = u;
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int prep_pow2ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

__global__ __launch_bounds__(PREP_NT) void prep_pcl_kernel(const float* __restrict__ img, const float* __restrict__ center, const double* __restrict__ Md,
                                                           const double* __restrict__ cube, const double* __restrict__ cam, const long long* __restrict__ seed, int S,
                                                           int n, int cap1, float* __restrict__ pcl, int* __restrict__ pcl_index, int* __restrict__ pcl_count,
                                                           float* __restrict__ cand_pts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // [cap1]: one element per candidate
  unsigned long long* pick = keys + cap1;                                  // [pow2ceil(n)]: the n output slots when the cloud is tiled
  int* wsum = reinterpret_cast<int*>(pick + prep_pow2ceil(n));             // [PREP_NW] wave totals, [PREP_NW]: number of keys kept by the pre-filter
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, P = S * S;
  const float* im = img + (size_t)b * P;
  PclGeom g;
  g.scale = Md[9 * b];
  g.m02 = Md[9 * b + 2];
  g.m12 = Md[9 * b + 5];
  g.fx = cam[4 * b];
  g.fy = cam[4 * b + 1];
  g.fu = cam[4 * b + 2];
  g.fv = cam[4 * b + 3];
  g.cx = (double)center[3 * b];
  g.cy = (double)center[3 * b + 1];
  g.cz = (double)center[3 * b + 2];
  g.cube2 = cube[3 * b + 2];
  g.hx = cube[3 * b] / 2.0;
  g.hy = cube[3 * b + 1] / 2.0;
  g.hz = cube[3 * b + 2] / 2.0;
  const unsigned base = prep_seed_base(seed[b]);
  PREP_STAMP(4);

  // 1. compaction in row-major order (np.where): thread t owns pixels [t * per, (t + 1) * per)
  const int per = (P + PREP_NT - 1) / PREP_NT, p0 = min(t * per, P), p1 = min(p0 + per, P);
  float pt[3];
  int mine = 0;
  for (int p = p0; p < p1; ++p) mine += prep_point(im[p], p / S, p % S, g, pt) ? 1 : 0;
  int inc = mine;  // inclusive scan over the wave, then over the waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wsum[wv] = inc;
  if (t == 0) wsum[PREP_NW] = 0;
  __syncthreads();
  int before = inc - mine, N = 0;
  for (int w = 0; w < PREP_NW; ++w) {
    const int s = wsum[w];
    if (w < wv) before += s;
    N += s;
  }
  // Only the n smallest keys are wanted.  With N > 2 n candidates, keep the keys under a threshold that 1.5 n of them are expected to pass (hash bits are
  // uniform: 1.5 n +- sqrt(1.5 n), so between n and 2 n) and sort those: the same n smallest in the same order, from a sort over 2 n elements instead of up
  // to 16 384 (in-kernel stamps: the sort was 146 of the 190 us of a full crop).  Fewer than n pass (never observed): every key is written and sorted.
  const bool filt = N > 2 * n;
  const unsigned long long thr = filt ? ((3ull * (unsigned long long)n) << 35) / (unsigned long long)N : 0ull;
  int cand = before;
  for (int p = p0; p < p1; ++p)
    if (prep_point(im[p], p / S, p % S, g, pt)) {
      const unsigned long long key = prep_key(base, (unsigned)cand, 0x243f6a88U, (unsigned)cand, (unsigned)p);
      if (!filt)
        keys[cand] = key;
      else if ((key >> 28) < thr)
        keys[atomicAdd(&wsum[PREP_NW], 1)] = key;  // (any order: the sort follows)
      if (cand_pts) {
        float* o = cand_pts + ((size_t)b * P + cand) * 3;
        o[0] = pt[0];
        o[1] = pt[1];
        o[2] = pt[2];
      }
      ++cand;
    }
  if (t == 0) pcl_count[b] = N;
  float* out = pcl + (size_t)b * n * 3;
  int* oidx = pcl_index + (size_t)b * n;
  if (N == 0) {  // (N is the same in every thread: the branches below are workgroup-uniform)
    for (int i = t; i < n; i += PREP_NT) {
      out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = 0.f;
      oidx[i] = -1;
    }
    PREP_STAMP(5);
    PREP_STAMP(6);
    PREP_STAMP(7);
    return;
  }
  int K = N;  // keys to sort
  if (filt) {
    __syncthreads();
    K = wsum[PREP_NW];
    if (K < n) {  // (workgroup-uniform) the threshold kept too few: all keys
      cand = before;
      for (int p = p0; p < p1; ++p)
        if (prep_point(im[p], p / S, p % S, g, pt)) {
          keys[cand] = prep_key(base, (unsigned)cand, 0x243f6a88U, (unsigned)cand, (unsigned)p);
          ++cand;
        }
      K = N;
    }
  }
  const int P1 = prep_pow2ceil(K);
  for (int i = K + t; i < P1; i += PREP_NT) keys[i] = ~0ull;
  __syncthreads();
  PREP_STAMP(5);
  const unsigned long long* src = keys;
  if (N >= n) {
    // 2a. n of N without replacement in random order: the n smallest keys, in key order
    prep_bitonic_sort(keys, P1);
  } else {
    // 2b. sample_points' multiset: every candidate floor(n / N) times, n mod N distinct ones (the smallest keys) once more, then all n slots shuffled
    const int q = n / N, r = n - q * N;
    if (r > 0) prep_bitonic_sort(keys, P1);
    const int P2 = prep_pow2ceil(n);
    for (int i = t; i < P2; i += PREP_NT) {
      unsigned long long e = ~0ull;
      if (i < n) {
        const int copy = i < q * N ? i / N : q, j = i < q * N ? i - copy * N : i - q * N;  // j: position in keys (tiled part: all of them; extras: the first r)
        const unsigned pay = (unsigned)(keys[j] & 0xfffffffull), c = pay >> 14;
        e = prep_key(base, (unsigned)(copy * N) + c, 0x85a308d3U, c, pay & 0x3fffu);
      }
      pick[i] = e;
    }
    __syncthreads();
    prep_bitonic_sort(pick, P2);
    src = pick;
  }
  PREP_STAMP(6);
  // 3. the points of the chosen candidates
  for (int i = t; i < n; i += PREP_NT) {
    const unsigned pay = (unsigned)(src[i] & 0xfffffffull);
    const int c = (int)(pay >> 14), p = (int)(pay & 0x3fffu);
    prep_point(im[p], p / S, p % S, g, pt);
    out[3 * i] = pt[0];
    out[3 * i + 1] = pt[1];
    out[3 * i + 2] = pt[2];
    oidx[i] = c;
  }
  PREP_STAMP(7);
}

// project_to_crop + uncrop_points, one thread per joint, double inside (kpf_uncrop_joint of kpf_common.h, shared with kpf_track.hip)
__global__ __launch_bounds__(256) void prep_uncrop_kernel(const float* __restrict__ joints, const float* __restrict__ center, const float* __restrict__ M,
                                                          const float* __restrict__ cube, const float* __restrict__ cam, int B, int J, float* __restrict__ crop_px,
                                                          float* __restrict__ frame_px) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * J) return;
  const int b = e / J;
  kpf_uncrop_joint(joints + 3 * e, center + 3 * b, M + 9 * b, cube + 3 * b, cam + 4 * b, crop_px + 3 * e, frame_px + 3 * e);
}

// kpf_prep_uncrop_f32 for the samples of kpf_prep_annot_u16: a mirrored sample's frame u goes back to the camera's own frame (W - 1 - u, in double before the
// rounding to float); crop pixels, depths and every un-mirrored sample are the bits of prep_uncrop_kernel.  The predicted xyz stays in the MIRRORED camera's
// space, as in the reference, which scores left hands there.
__global__ __launch_bounds__(256) void prep_uncrop_mirror_kernel(const float* __restrict__ joints, const float* __restrict__ center, const float* __restrict__ M,
                                                                 const float* __restrict__ cube, const float* __restrict__ cam,
                                                                 const unsigned char* __restrict__ mirror, int frame_w, int B, int J,
                                                                 float* __restrict__ crop_px, float* __restrict__ frame_px) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * J) return;
  const int b = e / J;
  kpf_uncrop_joint(joints + 3 * e, center + 3 * b, M + 9 * b, cube + 3 * b, cam + 4 * b, crop_px + 3 * e, frame_px + 3 * e, mirror[b] ? (double)frame_w : -1.0);
}
#endif  // __HIPCC__

inline int host_pow2ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

// what the launchers of the three crop kernels check alike (has_joints: the dataset kernels, one lane per joint)
static int prep_crop_args(const char* name, int B, bool has_joints, int J, const int* frame_index, int F, int Hs, int Ws, int x0, int y0, int H, int W, int S) {
  KPF_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "%s: bad shape (B %d, window %d x %d, frame %d x %d)", name, B, Hs, Ws, H, W);
  KPF_REQUIRE(!has_joints || (J > 0 && J <= 64), "%s: J = %d joints (one lane of a wave64 per joint: 1 .. 64)", name, J);
  KPF_REQUIRE(F > 0 && (frame_index || F >= B), "%s: %d stored frames for %d samples%s", name, F, B, frame_index ? "" : " without a frame index");
  KPF_REQUIRE(x0 >= 0 && y0 >= 0 && x0 + Ws <= W && y0 + Hs <= H, "%s: the %d x %d window at (%d, %d) leaves the %d x %d frame", name, Ws, Hs, x0, y0, W, H);
  KPF_REQUIRE((long)Hs * Ws < (1L << 30), "%s: window of %d x %d pixels is too large", name, Hs, Ws);
  KPF_REQUIRE(S > 0 && S * S <= PREP_MAX_PIX, "%s: S = %d unsupported (S * S <= %d: the LDS plan of kpf_prep_pcl_sample)", name, S, PREP_MAX_PIX);
  return KPF_OK;
}

// the one launch behind kpf_prep_crop_u16 (frame_index NULL, F = B: sample b reads frame b) and kpf_prep_crop_u16_indexed
static int prep_crop_launch(const char* name, const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const double* bbox,
                            const double* cam, const double* cube, int B, int Hs, int Ws, int x0, int y0, int H, int W, int S, float* img, float* img_rgb,
                            float* center, float* M, float* cube_out, float* cam_para, double* com, int* bounds, double* M64, void* stream) {
  KPF_REQUIRE(rgb && depth && bbox && cam && cube && img && img_rgb && center && M && cube_out && cam_para && com && bounds && M64, "%s: null pointer argument", name);
  if (const int rc = prep_crop_args(name, B, false, 0, frame_index, F, Hs, Ws, x0, y0, H, W, S)) return rc;
  hipLaunchKernelGGL(prep_crop_kernel, dim3(B), dim3(PREP_NT), PREP_LDS_CROP.bytes(S), ST(stream), rgb, depth, frame_index, F, bbox, cam, cube, Hs, Ws, x0, y0, H, W, S,
                     img, img_rgb, center, M, cube_out, cam_para, com, bounds, M64);
  return kpf_check_launch(name);
}

extern "C" int kpf_prep_crop_u16(const unsigned char* rgb, const unsigned short* depth, const double* bbox, const double* cam, const double* cube, int B,
                                 int Hs, int Ws, int x0, int y0, int H, int W, int S, float* img, float* img_rgb, float* center, float* M, float* cube_out,
                                 float* cam_para, double* com, int* bounds, double* M64, void* stream) {
  return prep_crop_launch("kpf_prep_crop_u16", rgb, depth, nullptr, B, bbox, cam, cube, B, Hs, Ws, x0, y0, H, W, S, img, img_rgb, center, M, cube_out, cam_para,
                          com, bounds, M64, stream);
}

extern "C" int kpf_prep_crop_u16_indexed(const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const double* bbox,
                                         const double* cam, const double* cube, int B, int Hs, int Ws, int x0, int y0, int H, int W, int S, float* img,
                                         float* img_rgb, float* center, float* M, float* cube_out, float* cam_para, double* com, int* bounds, double* M64,
                                         void* stream) {
  KPF_REQUIRE(frame_index, "kpf_prep_crop_u16_indexed: null frame index (kpf_prep_crop_u16 is the entry without one)");
  return prep_crop_launch("kpf_prep_crop_u16_indexed", rgb, depth, frame_index, F, bbox, cam, cube, B, Hs, Ws, x0, y0, H, W, S, img, img_rgb, center, M, cube_out,
                          cam_para, com, bounds, M64, stream);
}

extern "C" int kpf_prep_pcl_sample(const float* img, const float* center, const double* M64, const double* cube, const double* cam, const long long* seed,
                                   int B, int S, int n, float* pcl, int* pcl_index, int* pcl_count, float* cand_pts, void* stream) {
  KPF_REQUIRE(img && center && M64 && cube && cam && seed && pcl && pcl_index && pcl_count, "kpf_prep_pcl_sample: null pointer argument");
  KPF_REQUIRE(B > 0, "kpf_prep_pcl_sample: B = %d", B);
  KPF_REQUIRE(S > 0 && S * S <= PREP_MAX_PIX, "kpf_prep_pcl_sample: S = %d unsupported (S * S <= %d: one 8-byte sort element per pixel in LDS)", S, PREP_MAX_PIX);
  KPF_REQUIRE(n > 0 && n <= S * S, "kpf_prep_pcl_sample: n = %d samples of at most S * S = %d pixels", n, S * S);
  const int cap1 = host_pow2ceil(S * S);
  const size_t lds = ((size_t)cap1 + host_pow2ceil(n)) * 8 + 2 * PREP_NW * 4;
  KPF_REQUIRE(lds <= 160 * 1024, "kpf_prep_pcl_sample: S = %d with n = %d needs %zu bytes of LDS (160 KiB per workgroup)", S, n, lds);
  static std::atomic<bool> raised[KPF_MAX_DEVICES];
  if (lds > 64 * 1024)
    KPF_REQUIRE(kpf_raise_lds_limit(reinterpret_cast<const void*>(prep_pcl_kernel), raised), "kpf_prep_pcl_sample: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL(prep_pcl_kernel, dim3(B), dim3(PREP_NT), lds, ST(stream), img, center, M64, cube, cam, seed, S, n, cap1, pcl, pcl_index, pcl_count, cand_pts);
  return kpf_check_launch("kpf_prep_pcl_sample");
}

extern "C" int kpf_prep_uncrop_f32(const float* joints, const float* center, const float* M, const float* cube, const float* cam, int B, int J, float* crop_px,
                                   float* frame_px, void* stream) {
  KPF_REQUIRE(joints && center && M && cube && cam && crop_px && frame_px, "kpf_prep_uncrop_f32: null pointer argument");
  KPF_REQUIRE(B > 0 && J > 0 && (long)B * J < (1L << 30), "kpf_prep_uncrop_f32: bad shape (B %d, J %d)", B, J);
  hipLaunchKernelGGL(prep_uncrop_kernel, dim3((B * J + 255) / 256), dim3(256), 0, ST(stream), joints, center, M, cube, cam, B, J, crop_px, frame_px);
  return kpf_check_launch("kpf_prep_uncrop_f32");
}

extern "C" int kpf_prep_annot_u16(const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const float* joints_mm, const float* cam32,
                                  const float* center_xyz, const unsigned char* mirror, const double* cube, int B, int J, int Hs, int Ws, int x0, int y0, int H,
                                  int W, int S, float* img, float* img_rgb, float* center, float* M, float* cube_out, float* cam_para, double* com, int* bounds,
                                  double* M64, float* joint, float* joint_img, double* cam64, void* stream) {
  const char* name = "kpf_prep_annot_u16";
  KPF_REQUIRE(rgb && depth && cam32 && mirror && cube && img && img_rgb && center && M && cube_out && cam_para && com && bounds && M64 && joint && joint_img && cam64,
              "%s: null pointer argument", name);
  KPF_REQUIRE(joints_mm || center_xyz, "%s: neither joints nor a centre (nothing to crop around)", name);
  if (const int rc = prep_crop_args(name, B, true, J, frame_index, F, Hs, Ws, x0, y0, H, W, S)) return rc;
  hipLaunchKernelGGL(prep_annot_kernel, dim3(B), dim3(PREP_NT), PREP_LDS_ANNOT.bytes(S), ST(stream), rgb, depth, frame_index, F, joints_mm, cam32, center_xyz, mirror, cube,
                     J, Hs, Ws, x0, y0, H, W, S, img, img_rgb, center, M, cube_out, cam_para, com, bounds, M64, joint, joint_img, cam64);
  return kpf_check_launch(name);
}

extern "C" int kpf_prep_uncrop_mirror_f32(const float* joints, const float* center, const float* M, const float* cube, const float* cam, const unsigned char* mirror,
                                          int frame_w, int B, int J, float* crop_px, float* frame_px, void* stream) {
  KPF_REQUIRE(joints && center && M && cube && cam && mirror && crop_px && frame_px, "kpf_prep_uncrop_mirror_f32: null pointer argument");
  KPF_REQUIRE(B > 0 && J > 0 && (long)B * J < (1L << 30), "kpf_prep_uncrop_mirror_f32: bad shape (B %d, J %d)", B, J);
  KPF_REQUIRE(frame_w > 0, "kpf_prep_uncrop_mirror_f32: frame width %d", frame_w);
  hipLaunchKernelGGL(prep_uncrop_mirror_kernel, dim3((B * J + 255) / 256), dim3(256), 0, ST(stream), joints, center, M, cube, cam, mirror, frame_w, B, J, crop_px,
                     frame_px);
  return kpf_check_launch("kpf_prep_uncrop_mirror_f32");
}

extern "C" int kpf_prep_augment_u16(const unsigned char* rgb, const unsigned short* depth, const int* frame_index, int F, const float* joints_mm, const float* cam32,
                                    const float* center_xyz, const unsigned char* mirror, const double* cube, const int* mode, const double* off, const double* sc,
                                    const double* rot, const double* rot_cs, const double* color, int B, int J, int Hs, int Ws, int x0, int y0, int H, int W, int S,
                                    float* img, float* img_rgb, float* center, float* M, float* cube_out, float* cam_para, double* com, int* bounds, double* M64,
                                    float* joint, float* joint_img, double* cam64, double* cube64, int* aug_status, void* stream) {
  const char* name = "kpf_prep_augment_u16";
  KPF_REQUIRE(rgb && depth && cam32 && mirror && cube && img && img_rgb && center && M && cube_out && cam_para && com && bounds && M64 && joint && joint_img && cam64 &&
                  cube64 && aug_status,
              "%s: null pointer argument", name);
  KPF_REQUIRE(joints_mm, "%s: null joints (a training item has labels)", name);
  KPF_REQUIRE(mode && off && sc && rot && rot_cs, "%s: null augmentation parameter (mode, off, sc, rot and rot_cs are required; color may be NULL)", name);
  if (const int rc = prep_crop_args(name, B, true, J, frame_index, F, Hs, Ws, x0, y0, H, W, S)) return rc;
  hipLaunchKernelGGL(prep_augment_kernel, dim3(B), dim3(PREP_NT), PREP_LDS_AUGMENT.bytes(S), ST(stream), rgb, depth, frame_index, F, joints_mm, cam32, center_xyz, mirror,
                     cube, mode, off, sc, rot, rot_cs, color, J, Hs, Ws, x0, y0, H, W, S, img, img_rgb, center, M, cube_out, cam_para, com, bounds, M64, joint, joint_img,
                     cam64, cube64, aug_status);
  return kpf_check_launch(name);
}

extern "C" int kpf_prep_aug_draw(long long* seed, int B, double sigma_com, double sigma_sc, double rot_range, double color_factor, long long seed_stride, int* mode,
                                 double* off, double* sc, double* rot, double* rot_cs, double* color, void* stream) {
  const char* name = "kpf_prep_aug_draw";
  KPF_REQUIRE(seed && mode && off && sc && rot && rot_cs && color, "%s: null pointer argument", name);
  KPF_REQUIRE(B > 0, "%s: B = %d", name, B);
  KPF_REQUIRE(sigma_com >= 0 && sigma_sc >= 0 && rot_range >= 0 && color_factor >= 0 && sigma_com - sigma_com == 0 && sigma_sc - sigma_sc == 0 &&
                  rot_range - rot_range == 0 && color_factor - color_factor == 0,
              "%s: sigma_com %g, sigma_sc %g, rot_range %g and color_factor %g must be finite and not negative", name, sigma_com, sigma_sc, rot_range, color_factor);
  hipLaunchKernelGGL(prep_aug_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, ST(stream), seed, B, sigma_com, sigma_sc, rot_range, color_factor, seed_stride, mode, off,
                     sc, rot, rot_cs, color);
  return kpf_check_launch(name);
}

/* tuning aid: [B][8] 8-byte stamp slots in device memory for the next launches (NULL switches the stamps off) */
extern "C" int kpf_prep_set_stamps(void* p) {
  unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
  if (hipMemcpyToSymbol(HIP_SYMBOL(kpf_prep_stamps), &q, sizeof(q)) != hipSuccess) {
    kpf_set_error("kpf_prep_set_stamps: cannot set the device symbol");
    return KPF_ELAUNCH;
  }
  return KPF_OK;
}
