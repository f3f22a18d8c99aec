// The mesh object, as the four files that work on it see it: mesh.hip (the object itself and the strokes), mesh_bleed.hip (coverage and
// the bleed pass), mesh_pick.hip (picking) and topology.hip (growing a face set).  Private to them: every other file reaches a mesh
// through mesh_geom (mesh_dev.h).
#pragma once
#include "mesh_dev.h"
#include "mesh_host.h"
#include "stamp.h"

enum { MF_RASTER = 1, MF_FRONT = 2, MF_UPRIGHT = 4 };  // finite with a non-zero area; unit normal z >= 0; >= 0.5 (not steep)

// what one stamp's projection leaves per face: window position snapped to 1/256 pixel, camera z, NDC (the backprojection's feature)
struct FaceRec { int X[3], Y[3]; float z[3], nx[3], ny[3]; int flags; };
// per mesh, on the device: the faces that can cover a pixel centre of the window, those that are backprojected, and the texel bounding box
// of the latter (x0, y0, x1, y1); n_big: the faces a coverage build hands to its tile pass
struct MeshState { int n_win, n_val, bb[4], n_big; };
struct PickRay;  // mesh_pick.hip

struct Mesh {
  Ctx* ctx = nullptr;
  int V = 0, F = 0;
  float* verts = nullptr;  // [V][3]
  int* faces = nullptr;    // [F][3]
  float* uvs = nullptr;    // [F][3][2]
  FaceRec* rec = nullptr;  // [F], of the last projection
  int* owned = nullptr;    // [F]: the face won at least one pixel of the last render
  int4* win = nullptr;     // [F] {face, px0 | px1 << 16, py0 | py1 << 16, 0}
  int4* val = nullptr;     // [F] the same in texels
  MeshState* state = nullptr;
  // the texels of a cov_H x cov_W texture that any face covers, 1 bit per texel in rows of (cov_W + 31) / 32 words, followed by the
  // table of bleed offsets (2 * MESH_MAX_OFF bytes); built at the first use of a size, one per mesh (mesh_bleed.hip)
  unsigned int* cov = nullptr;
  int cov_H = 0, cov_W = 0;
  double lo[3], hi[3];     // the vertices' bounding box (host): a window it misses is skipped without a launch
  // picking (mesh_pick.hip): allocated at the first pick, in steps of PICK_CHUNK rays; no stroke reads or writes them
  PickRay* pick_rays = nullptr;               // [pick_cap]
  unsigned long long* pick_slots = nullptr;   // [pick_cap]: the winner's (order-preserving bits of z) << 32 | ~face; 0: no hit
  dtp_mesh_hit* pick_out = nullptr;           // [pick_cap]
  char* pick_host = nullptr;                  // pinned: [pick_cap] PickRay, then [pick_cap] dtp_mesh_hit
  int pick_cap = 0;
  int* sel_poly = nullptr;  // [2 * 1024]: the snapped polygon of the lasso in flight (select.hip); no stroke, pick or view touches it
  void* view = nullptr;  // the buffers of dtp_mesh_view (view.hip): allocated at the first view; no stroke or pick touches them
  void* topo = nullptr;  // the topology and the scratch of dtp_mesh_select_extend (topology.hip): built at the first use
};

bool mesh_alive(const Mesh* m);  // mesh.hip, as the next two: a destroyed handle is refused, not followed
int check_texture(const char* who, const void* texture, int H, int W);
int check_bleed(const char* who, int bleed);
int ensure_coverage(Mesh* m, int H, int W, hipStream_t s);  // mesh_bleed.hip, as the next
int enqueue_bleed(Mesh* m, unsigned char* texture, int H, int W, int k, const int* rect, hipStream_t s);

inline int launch_ok() { return hipGetLastError() == hipSuccess ? DTP_OK : DTP_ERR_HIP; }
// What most entry points open with.  given: the other required pointers are there; list: what the message says of them.  An entry point
// with checks of its own between the two refusals has made the first itself and passes a mesh that is not null.
inline int check_mesh(const char* who, const Mesh* m, bool given = true, const char* list = "") {
  if (!m || !given) { dtp_set_error("%s: NULL argument%s", who, list); return DTP_ERR_ARG; }
  if (!mesh_alive(m)) { dtp_set_error("%s: the mesh is not a live mesh (destroyed?)", who); return DTP_ERR_ARG; }
  return DTP_OK;
}
