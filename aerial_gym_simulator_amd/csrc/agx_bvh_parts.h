// Pieces of the LBVH builders shared by the LDS-resident build (agx_scene.hip) and the global-memory build of scenes above
// its cap (agx_scene_large.hip): key construction, the radix tree's prefix length, the recognition of box objects.
#pragma once
#include "agx_common.h"
#include "agx_device_math.h"

namespace agx {

constexpr float kBoxEps = 1.0e-3f;

constexpr float kBvhLargeFraction = 0.75f;

// obstacle parked outside the env by the curriculum (asset_manager.py:71 puts it at -1000 m)
AGX_DEV bool tri_parked(const float *t) { return t[0] < -900.0f && t[1] < -900.0f && t[2] < -900.0f; }

AGX_DEV uint32_t expand_bits10(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

AGX_DEV int delta_keys(const unsigned long long *keys, int nt, int i, int j) {
  if (j < 0 || j >= nt) return -1;
  return __clzll(keys[i] ^ keys[j]);  // keys are unique (the triangle index is in the low word)
}

// AGX_BVH_BOX_OBJECTS.  An internal node whose leaves are exactly ONE object's 12 triangles becomes an OBJECT NODE if those triangles
// make an orthogonal box of trimesh.creation.box's topology -- decided from the world-frame triangles alone, every vertex checked,
// in three parallel steps (a thread that validated an object alone was a chain of ~120 dependent loads: +20 us on a 60 us build):
//   1. per internal node: is its key range one object's twelve keys?  (LDS only)              -> objroot[object] = node
//   2. per triangle: are its three vertices corners of its object's box, in the plane of the face the ray-cast's table expects it
//      in; per face pair: do the two triangles have four distinct corners between them (they tile the rectangle)?  -> objroot[o] = -1
//   3. per object: the verdict into bit 0 of counter[node] (read by the node itself and by its parent in the emit stage).
// Faces of trimesh's box (corners ({0,1}^3 - 0.5) * extents, index 4 x + 2 y + z) by triangle:
//   0 = (1, 3, 0), 1 = (4, 1, 0), 2 = (0, 3, 2), 11 = (7, 5, 6);  -x (0, 2)  +x (10, 11)  -y (1, 5)  +y (7, 9)  -z (3, 8)  +z (4, 6).
struct BoxFrame {
  V3 nx, ny, nz, cen;
  float hx, hy, hz, tol;
};

// the box four corners of an object's first triangles span (corners 0, 1, 2, 4; the opposite corner 7 must close it)
AGX_DEV bool box_frame(const float *__restrict__ t, BoxFrame &F) {
  const V3 v1 = V3{t[0], t[1], t[2]}, v0 = V3{t[6], t[7], t[8]};          // triangle 0 = (1, 3, 0)
  const V3 v4 = V3{t[9], t[10], t[11]};                                     // triangle 1 = (4, 1, 0)
  const V3 v2 = V3{t[18 + 6], t[18 + 7], t[18 + 8]};                        // triangle 2 = (0, 3, 2)
  const V3 v7 = V3{t[99], t[100], t[101]};                                  // triangle 11 = (7, 5, 6)
  const V3 ex = v4 - v0, ey = v2 - v0, ez = v1 - v0;
  const float lx = sqrtf(dot(ex, ex)), ly = sqrtf(dot(ey, ey)), lz = sqrtf(dot(ez, ez));
  if (!(lx > 1.0e-5f && ly > 1.0e-5f && lz > 1.0e-5f) || !(lx < 1.0e4f && ly < 1.0e4f && lz < 1.0e4f)) return false;
  F.nx = ex * (1.0f / lx); F.ny = ey * (1.0f / ly); F.nz = ez * (1.0f / lz);
  if (fabsf(dot(F.nx, F.ny)) > 1.0e-4f || fabsf(dot(F.ny, F.nz)) > 1.0e-4f || fabsf(dot(F.nz, F.nx)) > 1.0e-4f) return false;
  const V3 far = v0 + ex + ey + ez - v7;  // the opposite corner is where a box has it
  if (!(sqrtf(dot(far, far)) <= 1.0e-4f * (lx + ly + lz))) return false;
  F.cen = v0 + (ex + ey + ez) * 0.5f;
  F.hx = 0.5f * lx; F.hy = 0.5f * ly; F.hz = 0.5f * lz;
  F.tol = 1.0e-4f * (lx + ly + lz) + 1.0e-5f;
  return true;
}

// triangle q of the object (9 floats at t): three distinct corners of the box, all in the plane of face `kFaceOf[q]`; -> the corners' ids
AGX_DEV bool box_triangle_ok(const BoxFrame &F, const float *__restrict__ t, int q, uint32_t &ids) {
  const int face = (int)((0x113435254020ull >> (4 * q)) & 15ull);  // {0, 2, 0, 4, 5, 2, 5, 3, 4, 3, 1, 1}[q] = 2 * axis + (plus side)
  const int axis = face >> 1;
  const float want = (face & 1) ? 1.0f : -1.0f;
  ids = 0u;
  bool ok = true;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const V3 p = V3{t[3 * v] - F.cen.x, t[3 * v + 1] - F.cen.y, t[3 * v + 2] - F.cen.z};
    const float l0 = dot(F.nx, p), l1 = dot(F.ny, p), l2 = dot(F.nz, p);
    ok = ok && !(fabsf(fabsf(l0) - F.hx) > F.tol || fabsf(fabsf(l1) - F.hy) > F.tol || fabsf(fabsf(l2) - F.hz) > F.tol);
    const float la = axis == 0 ? l0 : (axis == 1 ? l1 : l2);
    ok = ok && (la * want > 0.0f);
    ids |= 1u << ((l0 > 0.0f ? 4 : 0) | (l1 > 0.0f ? 2 : 0) | (l2 > 0.0f ? 1 : 0));
  }
  return ok && __popc(ids) == 3;
}

// the object node's record (include/aerial_gym_hip.h): the frame of object `obj`
AGX_DEV void box_object_record(const float *__restrict__ tris, int obj, float *rec) {
  BoxFrame F;
  box_frame(tris + (size_t)obj * 12 * 9, F);  // (validated before)
  rec[0] = F.nx.x; rec[1] = F.nx.y; rec[2] = F.nx.z; rec[3] = F.hx;
  rec[4] = F.ny.x; rec[5] = F.ny.y; rec[6] = F.ny.z; rec[7] = F.hy;
  rec[8] = F.nz.x; rec[9] = F.nz.y; rec[10] = F.nz.z; rec[11] = F.hz;
  rec[12] = F.cen.x; rec[13] = F.cen.y; rec[14] = F.cen.z; rec[15] = __int_as_float(obj * 12);
}

// mask -> work list (work[0] = count, work[1] = cursor, work[2 ...] = dirty env ids): k_compact_mask of agx_scene.hip
int compact_mask_launch(int n, const uint8_t *mask, int32_t *work, void *stream);

}  // namespace agx
