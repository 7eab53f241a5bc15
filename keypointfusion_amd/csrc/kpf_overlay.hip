// The result drawn over the frame on the device (overlay.FrameOverlay): the fitted meshes of every hand of a camera frame, shaded and
// depth-tested against each other and against the observed depth, and the skeletons over them.
//   kpf_overlay_project_f32   per hand: the vertices' grid coordinates, 1 / z, shade and the hand's pixel rectangle
//   kpf_overlay_draw_u8       per 64 x 64 tile of a stored frame: z-buffer in LDS over all hands of the frame, blend, skeleton, label / owner / prim / depth
// The edge rule and the depth at a pixel are kpf_mano_raster_f32's (kpf_raster_dev.h).  Every operation is individually rounded and every decision that
// depends on arrival order goes through an integer min: keypointfusion_amd/overlay.py::draw_host gives the same bits.
#include "kpf_raster_dev.h"

namespace {

constexpr int OV_NV = RASTER_NV;
constexpr int OV_TILE = 64, OV_TILE_PIX = OV_TILE * OV_TILE;  // 4096 64-bit keys: 32 KiB of LDS
constexpr int OV_MAXF = 2048, OV_MAXJ = 64, OV_MAXBONES = 64, OV_MAXHANDS = 1 << 20;  // the key's tag is hand << 11 | face: 31 bits

// ---------------------------------------------------------------------------------------------------------------
// Launch 1: one workgroup per hand.  U, V, sx, sy, iz are the crop render's expressions with sample_offset in place of its 0.5.
// ---------------------------------------------------------------------------------------------------------------
struct OverlayProjectArgs {
  const float *verts, *normals, *cam, *M;  // [B][778][3], the same or null, [B][4], [B][2][3] or null
  float sample_offset, ambient;
  int H, W;
  float *sx, *sy, *iz, *shade;             // [B][778]
  int *ok, *rect;                          // [B][778], [B][4]
};

__global__ __launch_bounds__(256) void overlay_project_kernel(OverlayProjectArgs a) {
#pragma clang fp contract(off)
  __shared__ float red[4][4];
  const int b = blockIdx.x, t = threadIdx.x;
  const float fx = a.cam[b * 4 + 0], fy = a.cam[b * 4 + 1], u0 = a.cam[b * 4 + 2], v0 = a.cam[b * 4 + 3];
  float m[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  if (a.M)
    for (int k = 0; k < 6; ++k) m[k] = a.M[b * 6 + k];
  const float rest = __fsub_rn(1.0f, a.ambient);
  float lox = INFINITY, loy = INFINITY, hix = -INFINITY, hiy = -INFINITY;  // over this thread's ok vertices; fminf / fmaxf skip a NaN
  for (int v = t; v < OV_NV; v += 256) {
    const long o = (long)b * OV_NV + v;
    const float x = a.verts[o * 3 + 0], y = a.verts[o * 3 + 1], z = a.verts[o * 3 + 2];
    const float U = __fadd_rn(__fdiv_rn(__fmul_rn(x, fx), z), u0), V = __fadd_rn(__fdiv_rn(__fmul_rn(y, fy), z), v0);
    const float sx = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], U), __fmul_rn(m[1], V)), m[2]), a.sample_offset);
    const float sy = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[3], U), __fmul_rn(m[4], V)), m[5]), a.sample_offset);
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && z > 0.0f;
    float shade = 1.0f;
    if (a.normals) {  // a headlight, two-sided: the mesh is open at the wrist
      const float nx = a.normals[o * 3 + 0], ny = a.normals[o * 3 + 1], nz = a.normals[o * 3 + 2];
      const bool some = isfinite(nx) && isfinite(ny) && isfinite(nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
      shade = some ? __fadd_rn(a.ambient, __fmul_rn(rest, fabsf(nz))) : a.ambient;
    }
    a.sx[o] = sx;
    a.sy[o] = sy;
    a.iz[o] = __fdiv_rn(1.0f, z);
    a.shade[o] = shade;
    a.ok[o] = ok ? 1 : 0;
    if (ok) {
      lox = fminf(lox, sx); hix = fmaxf(hix, sx);
      loy = fminf(loy, sy); hiy = fmaxf(hiy, sy);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // minima and maxima are exact: their order does not matter
    lox = fminf(lox, __shfl_xor(lox, o, 64)); hix = fmaxf(hix, __shfl_xor(hix, o, 64));
    loy = fminf(loy, __shfl_xor(loy, o, 64)); hiy = fmaxf(hiy, __shfl_xor(hiy, o, 64));
  }
  if ((t & 63) == 0) {
    red[t >> 6][0] = lox; red[t >> 6][1] = loy; red[t >> 6][2] = hix; red[t >> 6][3] = hiy;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) {
      lox = fminf(lox, red[w][0]); loy = fminf(loy, red[w][1]);
      hix = fmaxf(hix, red[w][2]); hiy = fmaxf(hiy, red[w][3]);
    }
    // clamped in float before the conversion: the low ends to [0, W] and [0, H], the high ends to [-1, W - 1] and [-1, H - 1], so that a hand with no ok
    // vertex (+inf, -inf) or one that lies off the grid has an empty rectangle
    a.rect[b * 4 + 0] = (int)fminf(fmaxf(ceilf(lox), 0.0f), (float)a.W);
    a.rect[b * 4 + 1] = (int)fminf(fmaxf(ceilf(loy), 0.0f), (float)a.H);
    a.rect[b * 4 + 2] = (int)fmaxf(fminf(floorf(hix), (float)(a.W - 1)), -1.0f);
    a.rect[b * 4 + 3] = (int)fmaxf(fminf(floorf(hiy), (float)(a.H - 1)), -1.0f);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 2: one workgroup per tile and stored frame.  Pass A renders every hand of the frame into the tile's z-buffer (the crop render's small-face /
// queued-face scheme, the pixel boxes clamped to the tile); pass B finds each pixel's last covering skeleton primitive; pass C writes the pixel.  A
// thread owns the tile's column t & 63 in the rows (t >> 6) + 4 i: a wave's loads and stores of a row are contiguous.
// ---------------------------------------------------------------------------------------------------------------
struct OverlayDrawArgs {
  const float *sx, *sy, *iz, *shade;  // [B][778], launch 1's; sx null: no mesh
  const int *ok, *rect, *faces;       // [B][778], [B][4], [Fc][3]
  const float* mesh_color;            // [B][3]
  const unsigned char* mesh_on;       // [B] or null
  const int* frame_index;             // [B] or null
  const unsigned char* rgb;           // [F][H][W][3]
  const unsigned short* depth_frame;  // [F][H][W] or null
  const float* joints_px;             // [B][J][3] or null: no skeleton
  const unsigned char* skel_on;       // [B] or null
  unsigned char *out, *label;         // [F][H][W][3], [F][H][W] or null
  int *owner, *prim;                  // [F][H][W] or null
  float* depth;                       // [F][H][W] or null
  int B, F, H, W, Fc, J, NB, tiles_x;
  float occl_margin, alpha, joint_radius, bone_half_width;
  unsigned char bones[OV_MAXBONES][2], bone_color[OV_MAXBONES][3], joint_color[OV_MAXJ][3];  // the skeleton's tables travel with the launch
};

__device__ __forceinline__ int overlay_frame_of(const OverlayDrawArgs& a, int b) {
  if (!a.frame_index) return b;
  const int f = a.frame_index[b];
  return f < 0 ? 0 : (f >= a.F ? a.F - 1 : f);
}

__device__ __forceinline__ unsigned char overlay_byte(float v) {  // floor(v + 0.5) clamped to 0..255, NaN -> 0 (fmaxf skips it)
#pragma clang fp contract(off)
  return (unsigned char)(int)fminf(fmaxf(floorf(__fadd_rn(v, 0.5f)), 0.0f), 255.0f);
}

constexpr int OV_BONE_BIT = 64;  // a skeleton winner is hand << 7 | OV_BONE_BIT (a bone) | index, -1: none

__global__ __launch_bounds__(256) void overlay_draw_kernel(OverlayDrawArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long zb[OV_TILE_PIX];
  __shared__ unsigned short queue[OV_MAXF];
  __shared__ unsigned long long pmask[2];
  __shared__ float ju[OV_MAXJ], jv[OV_MAXJ];
  __shared__ int qcount;
  const int t = threadIdx.x, lane = t & 63, frame = blockIdx.y, H = a.H, W = a.W;
  const int tx0 = ((int)blockIdx.x % a.tiles_x) * OV_TILE, ty0 = ((int)blockIdx.x / a.tiles_x) * OV_TILE;
  const int tx1 = min(tx0 + OV_TILE - 1, W - 1), ty1 = min(ty0 + OV_TILE - 1, H - 1);  // partial tiles at the right and bottom edges
  for (int p = t; p < OV_TILE_PIX; p += 256) zb[p] = RASTER_EMPTY;

  // ---- pass A: the meshes.  Every condition on b is uniform over the workgroup.
  if (a.sx)
    for (int b = 0; b < a.B; ++b) {
      if (overlay_frame_of(a, b) != frame || (a.mesh_on && !a.mesh_on[b])) continue;
      const int* rc = a.rect + (long)b * 4;
      if (rc[2] < rc[0] || rc[3] < rc[1] || rc[0] > tx1 || rc[2] < tx0 || rc[1] > ty1 || rc[3] < ty0) continue;  // every face's box lies inside the rectangle
      if (t == 0) qcount = 0;
      __syncthreads();  // also orders the buffer's initialisation before the first hand
      const float *sx = a.sx + (long)b * OV_NV, *sy = a.sy + (long)b * OV_NV, *iz = a.iz + (long)b * OV_NV;
      const int* ok = a.ok + (long)b * OV_NV;
      const unsigned tag = (unsigned)b << 11;
      for (int k = t; k < a.Fc; k += 256) {  // a small face is walked by its thread, a large one is queued (at most Fc <= 2048 entries)
        RasterFace f;
        if (!f.set(a.faces, k, sx, sy, iz, ok, tx0, tx1, ty0, ty1)) continue;
        if ((f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) > RASTER_SMALL) {
          queue[atomicAdd(&qcount, 1)] = (unsigned short)k;
          continue;
        }
        for (int r = f.y0; r <= f.y1; ++r)
          for (int c = f.x0; c <= f.x1; ++c) raster_min(f, c, r, tag | (unsigned)k, &zb[(r - ty0) * OV_TILE + (c - tx0)]);
      }
      __syncthreads();
      const int nq = qcount;
      for (int q = t >> 6; q < nq; q += 4) {  // a queued face is walked by one wave, 8 x 8 pixels at a step
        const int k = queue[q];
        RasterFace f;
        f.set(a.faces, k, sx, sy, iz, ok, tx0, tx1, ty0, ty1);
        for (int r = f.y0 + (lane >> 3); r <= f.y1; r += 8)
          for (int c = f.x0 + (lane & 7); c <= f.x1; c += 8) raster_min(f, c, r, tag | (unsigned)k, &zb[(r - ty0) * OV_TILE + (c - tx0)]);
      }
      __syncthreads();  // the count is read before the next hand resets it
    }

  // ---- pass B: the skeletons, hands ascending, a hand's joints and then its bones: the last covering primitive stays
  const int c = tx0 + lane, rbase = ty0 + (t >> 6);
  const float pxf = (float)c;
  int win[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) win[i] = -1;
  if (a.joints_px) {
    const float R = a.joint_radius, R2 = __fmul_rn(R, R), hw = a.bone_half_width, hw2 = __fmul_rn(hw, hw);
    const float tlo_x = (float)tx0, thi_x = (float)tx1, tlo_y = (float)ty0, thi_y = (float)ty1;
    for (int b = 0; b < a.B; ++b) {
      if (overlay_frame_of(a, b) != frame || (a.skel_on && !a.skel_on[b])) continue;
      const float* jp = a.joints_px + (long)b * a.J * 3;
      __syncthreads();  // the previous hand's joints are read no more
      // a primitive's pixel box, part of the rule: one pixel beyond its extent.  Wave 0 culls the joints against the tile, wave 1 the bones.
      if (t < 64) {
        bool hit = false;
        if (t < a.J) {
          const float u = jp[t * 3 + 0], v = jp[t * 3 + 1];
          ju[t] = u;
          jv[t] = v;
          hit = isfinite(u) && isfinite(v) && __fsub_rn(__fsub_rn(u, R), 1.0f) <= thi_x && __fadd_rn(__fadd_rn(u, R), 1.0f) >= tlo_x &&
                __fsub_rn(__fsub_rn(v, R), 1.0f) <= thi_y && __fadd_rn(__fadd_rn(v, R), 1.0f) >= tlo_y;
        }
        const unsigned long long mask = __ballot(hit);
        if (t == 0) pmask[0] = mask;
      } else if (t < 128) {
        bool hit = false;
        if (lane < a.NB) {
          const int ia = a.bones[lane][0], ib = a.bones[lane][1];
          const float ax = jp[ia * 3 + 0], ay = jp[ia * 3 + 1], bx = jp[ib * 3 + 0], by = jp[ib * 3 + 1];
          hit = isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by) && __fsub_rn(__fsub_rn(fminf(ax, bx), hw), 1.0f) <= thi_x &&
                __fadd_rn(__fadd_rn(fmaxf(ax, bx), hw), 1.0f) >= tlo_x && __fsub_rn(__fsub_rn(fminf(ay, by), hw), 1.0f) <= thi_y &&
                __fadd_rn(__fadd_rn(fmaxf(ay, by), hw), 1.0f) >= tlo_y;
        }
        const unsigned long long mask = __ballot(hit);
        if (t == 64) pmask[1] = mask;
      }
      __syncthreads();
      for (unsigned long long m = pmask[0]; m; m &= m - 1) {  // the joints that meet the tile, ascending (the mask is uniform)
        const int j = __ffsll((long long)m) - 1;
        const float u = ju[j], v = jv[j];
        const float dx = __fsub_rn(pxf, u), dx2 = __fmul_rn(dx, dx);
        const bool inx = pxf >= __fsub_rn(__fsub_rn(u, R), 1.0f) && pxf <= __fadd_rn(__fadd_rn(u, R), 1.0f);
        const float ylo = __fsub_rn(__fsub_rn(v, R), 1.0f), yhi = __fadd_rn(__fadd_rn(v, R), 1.0f);
        const int code = (b << 7) | j;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pyf = (float)(rbase + 4 * i), dy = __fsub_rn(pyf, v);
          if (inx && pyf >= ylo && pyf <= yhi && __fadd_rn(dx2, __fmul_rn(dy, dy)) <= R2) win[i] = code;
        }
      }
      for (unsigned long long m = pmask[1]; m; m &= m - 1) {  // then the bones
        const int j = __ffsll((long long)m) - 1;
        const int ia = a.bones[j][0], ib = a.bones[j][1];
        const float ax = ju[ia], ay = jv[ia], bx = ju[ib], by = jv[ib];
        const float ex = __fsub_rn(bx, ax), ey = __fsub_rn(by, ay), L = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        const float px = __fsub_rn(pxf, ax);
        const bool inx = pxf >= __fsub_rn(__fsub_rn(fminf(ax, bx), hw), 1.0f) && pxf <= __fadd_rn(__fadd_rn(fmaxf(ax, bx), hw), 1.0f);
        const float ylo = __fsub_rn(__fsub_rn(fminf(ay, by), hw), 1.0f), yhi = __fadd_rn(__fadd_rn(fmaxf(ay, by), hw), 1.0f);
        const int code = (b << 7) | OV_BONE_BIT | j;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pyf = (float)(rbase + 4 * i), py = __fsub_rn(pyf, ay);
          const float tt = L > 0.0f ? fminf(fmaxf(__fdiv_rn(__fadd_rn(__fmul_rn(px, ex), __fmul_rn(py, ey)), L), 0.0f), 1.0f) : 0.0f;
          const float qx = __fsub_rn(px, __fmul_rn(tt, ex)), qy = __fsub_rn(py, __fmul_rn(tt, ey));
          if (inx && pyf >= ylo && pyf <= yhi && __fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)) <= hw2) win[i] = code;
        }
      }
    }
  }
  __syncthreads();  // pass A's keys are complete (no hand may have passed its barriers)

  // ---- pass C: the pixels
  if (c > tx1) return;
  const float keep = __fsub_rn(1.0f, a.alpha);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = rbase + 4 * i;
    if (r > ty1) break;
    const long g = ((long)frame * H + r) * W + c;
    const unsigned long long key = zb[(r - ty0) * OV_TILE + lane];
    unsigned char o0 = a.rgb[g * 3 + 0], o1 = a.rgb[g * 3 + 1], o2 = a.rgb[g * 3 + 2];
    int lab = 0, own = -1, pr = -1;
    float dep = 0.0f;
    if (key != RASTER_EMPTY) {
      const float d = __uint_as_float((unsigned)(key >> 32));
      const int hb = (int)((unsigned)key >> 11), k = (int)((unsigned)key & 2047u);
      dep = d; own = hb; pr = k;
      const unsigned short seen = a.depth_frame ? a.depth_frame[g] : (unsigned short)0;
      if (seen != 0 && (float)seen < __fsub_rn(d, a.occl_margin)) {
        lab = 4;  // hidden by the scene: the frame's pixel stays
      } else {
        lab = 1;
        RasterFace f;  // the winner's weights again, at this pixel
        f.set(a.faces, k, a.sx + (long)hb * OV_NV, a.sy + (long)hb * OV_NV, a.iz + (long)hb * OV_NV, a.ok + (long)hb * OV_NV, tx0, tx1, ty0, ty1);
        const float* sh = a.shade + (long)hb * OV_NV;
        const float s = f.interpolate(c, r, sh[f.i0], sh[f.i1], sh[f.i2]);
        const float* mc = a.mesh_color + (long)hb * 3;
        o0 = overlay_byte(__fadd_rn(__fmul_rn(keep, (float)o0), __fmul_rn(a.alpha, __fmul_rn(mc[0], s))));
        o1 = overlay_byte(__fadd_rn(__fmul_rn(keep, (float)o1), __fmul_rn(a.alpha, __fmul_rn(mc[1], s))));
        o2 = overlay_byte(__fadd_rn(__fmul_rn(keep, (float)o2), __fmul_rn(a.alpha, __fmul_rn(mc[2], s))));
      }
    }
    if (win[i] >= 0) {  // the skeleton lies over the mesh, opaque and without a depth test; the model depth stays the mesh's
      const int j = win[i] & 63;
      const bool bone = (win[i] & OV_BONE_BIT) != 0;
      const unsigned char* col = bone ? a.bone_color[j] : a.joint_color[j];
      o0 = col[0]; o1 = col[1]; o2 = col[2];
      lab = bone ? 2 : 3;
      own = win[i] >> 7;
      pr = j;
    }
    a.out[g * 3 + 0] = o0; a.out[g * 3 + 1] = o1; a.out[g * 3 + 2] = o2;
    if (a.label) a.label[g] = (unsigned char)lab;
    if (a.owner) a.owner[g] = own;
    if (a.prim) a.prim[g] = pr;
    if (a.depth) a.depth[g] = dep;
  }
}

}  // namespace

extern "C" int kpf_overlay_project_f32(const float* verts, const float* normals, const float* cam, const float* M, float sample_offset, float ambient, int H,
                                       int W, float* sx, float* sy, float* iz, float* shade, int* ok, int* rect, int B, void* stream) {
  const char* name = "kpf_overlay_project_f32";
  KPF_REQUIRE(verts && cam && sx && sy && iz && shade && ok && rect, "%s: null pointer", name);
  KPF_REQUIRE(B > 0 && B < OV_MAXHANDS && H >= 1 && W >= 1, "%s: bad shape B=%d H=%d W=%d (1 <= B < %d; 1 <= H, W)", name, B, H, W, OV_MAXHANDS);
  KPF_REQUIRE(ambient >= 0.f && ambient <= 1.f, "%s: ambient=%g outside [0, 1]", name, ambient);
  KPF_REQUIRE(isfinite(sample_offset), "%s: sample_offset=%g is not finite", name, sample_offset);
  OverlayProjectArgs a;
  a.verts = verts; a.normals = normals; a.cam = cam; a.M = M; a.sample_offset = sample_offset; a.ambient = ambient; a.H = H; a.W = W;
  a.sx = sx; a.sy = sy; a.iz = iz; a.shade = shade; a.ok = ok; a.rect = rect;
  hipLaunchKernelGGL(overlay_project_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}

extern "C" int kpf_overlay_draw_u8(const kpf_overlay_draw_desc* d, void* stream) {
  const char* name = "kpf_overlay_draw_u8";
  KPF_REQUIRE(d, "%s: null descriptor", name);
  KPF_REQUIRE(d->rgb && d->out, "%s: null pointer (rgb, out)", name);
  KPF_REQUIRE(d->B > 0 && d->B < OV_MAXHANDS && d->F >= 1 && d->F <= 65535 && d->H >= 1 && d->W >= 1,
              "%s: bad shape B=%d F=%d H=%d W=%d (1 <= B < %d; 1 <= F <= 65535; 1 <= H, W)", name, d->B, d->F, d->H, d->W, OV_MAXHANDS);
  KPF_REQUIRE(d->frame_index || d->F == d->B, "%s: without frame_index hand b lies on frame b, so F=%d must equal B=%d", name, d->F, d->B);
  const long tiles_x = ((long)d->W + OV_TILE - 1) / OV_TILE, tiles_y = ((long)d->H + OV_TILE - 1) / OV_TILE;
  KPF_REQUIRE(tiles_x * tiles_y <= 0x7fffffffL, "%s: too many tiles for H=%d W=%d", name, d->H, d->W);
  KPF_REQUIRE(d->alpha >= 0.f && d->alpha <= 1.f, "%s: alpha=%g outside [0, 1]", name, d->alpha);
  KPF_REQUIRE(isfinite(d->occl_margin), "%s: occl_margin=%g is not finite", name, d->occl_margin);
  if (d->sx) {
    KPF_REQUIRE(d->sy && d->iz && d->shade && d->ok && d->rect && d->faces && d->mesh_color, "%s: null pointer among the mesh's inputs", name);
    KPF_REQUIRE(d->Fc >= 1 && d->Fc <= OV_MAXF, "%s: Fc=%d outside 1..%d", name, d->Fc, OV_MAXF);
  }
  if (d->joints_px) {
    KPF_REQUIRE(d->J >= 1 && d->J <= OV_MAXJ && d->NB >= 0 && d->NB <= OV_MAXBONES, "%s: bad skeleton J=%d NB=%d (1 <= J <= %d; 0 <= NB <= %d)", name, d->J,
                d->NB, OV_MAXJ, OV_MAXBONES);
    KPF_REQUIRE(d->joint_color && (d->NB == 0 || (d->bones && d->bone_color)), "%s: null pointer among the skeleton's tables", name);
    KPF_REQUIRE(isfinite(d->joint_radius) && d->joint_radius >= 0.f, "%s: joint_radius=%g is negative or not finite", name, d->joint_radius);
    KPF_REQUIRE(isfinite(d->bone_half_width) && d->bone_half_width >= 0.f, "%s: bone_half_width=%g is negative or not finite", name, d->bone_half_width);
    for (int i = 0; i < d->NB * 2; ++i)
      KPF_REQUIRE(d->bones[i] >= 0 && d->bones[i] < d->J, "%s: bone %d ends at joint %d, outside [0, %d)", name, i / 2, d->bones[i], d->J);
  }
  {
    const uintptr_t in = reinterpret_cast<uintptr_t>(d->rgb), out = reinterpret_cast<uintptr_t>(d->out);
    const uintptr_t bytes = (uintptr_t)d->F * d->H * d->W * 3;
    KPF_REQUIRE(out + bytes <= in || in + bytes <= out, "%s: out overlaps rgb", name);
  }
  OverlayDrawArgs a = {};  // the unused rows of the skeleton's tables are zero
  a.sx = d->sx; a.sy = d->sy; a.iz = d->iz; a.shade = d->shade; a.ok = d->ok; a.rect = d->rect; a.faces = d->faces; a.mesh_color = d->mesh_color;
  a.mesh_on = d->mesh_on; a.frame_index = d->frame_index; a.rgb = d->rgb; a.depth_frame = d->depth_frame; a.joints_px = d->joints_px;
  a.skel_on = d->skel_on; a.out = d->out; a.label = d->label; a.owner = d->owner; a.prim = d->prim; a.depth = d->depth;
  a.B = d->B; a.F = d->F; a.H = d->H; a.W = d->W; a.Fc = d->sx ? d->Fc : 0; a.J = d->joints_px ? d->J : 0; a.NB = d->joints_px ? d->NB : 0;
  a.tiles_x = (int)tiles_x;
  a.occl_margin = d->occl_margin; a.alpha = d->alpha; a.joint_radius = d->joint_radius; a.bone_half_width = d->bone_half_width;
  for (int i = 0; i < a.NB; ++i) {
    a.bones[i][0] = (unsigned char)d->bones[i * 2 + 0];
    a.bones[i][1] = (unsigned char)d->bones[i * 2 + 1];
    for (int k = 0; k < 3; ++k) a.bone_color[i][k] = d->bone_color[i * 3 + k];
  }
  for (int i = 0; i < a.J * 3; ++i) a.joint_color[i / 3][i % 3] = d->joint_color[i];
  hipLaunchKernelGGL(overlay_draw_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)d->F), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return kpf_check_launch(name);
}
