// gs_tsdf.hip -- TSDF fusion of rendered depth maps (gsplat_tsdf_integrate; gsplat_tsdf_integrate_surface for maps that
// hold the surface depth itself) and the extraction of the zero level set as an indexed triangle mesh by marching
// tetrahedra (gsplat_tsdf_mark, gsplat_tsdf_emit); definitions: include/gsplat_hip.h.
//
// Like gs_normal.hip, every decision and every value is evaluated in double from the float inputs and rounded to float
// once.  Every kernel GATHERS: a thread owns a grid node (x on the lanes: a wave's loads and stores of the volume are one
// contiguous run of a row, and neighbouring nodes project to neighbouring pixels), nothing is added with atomics, two
// runs give the same bits.
//
// Integration keeps a node's running (tsdf, weight, colour) in registers over up to kTsdfViews views per pass: the volume
// is read and written once per pass, not once per view, and since the state is rounded to float after every view exactly
// as a store and a load would round it, a batch is bit for bit the same as its views one call at a time.  The cameras of a
// pass travel in the kernel's argument block (uniform loads).
//
// Extraction is count / scan / emit.  The Freudenthal split cuts every cell into the six tetrahedra {0, a, a|b, 7} (corners
// numbered by bits x = 1, y = 2, z = 4; (a, b, c) the orderings of the axes), which all share the body diagonal and cut
// every face along the diagonal from its low to its high corner: neighbouring cells agree on every shared face.  A vertex
// lives on a grid edge (lower node, one of seven directions), so it is named by (node, edge type) and found again by every
// triangle around it through the node's offset and the rank of the edge's bit in the node's edge mask: an indexed mesh
// without a welding pass, a sort or an atomic.
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int kTsdfViews = 8;       // views per pass over the volume
constexpr int kTX = 64, kTY = 4;    // a block: 64 nodes along x (one wave per row) by 4 rows of y

struct TsdfView { float m[12]; float fx, fy, cx, cy; };  // row-major [R|t], pixel intrinsics
struct TsdfBatch { TsdfView v[kTsdfViews]; int n; };
struct TsdfVolume { double ox, oy, oz, voxel; int nx, ny, nz; };
// inverse: kTsdfExpected (depth = sum alpha T z), kTsdfInverse (sum alpha T / z), kTsdfSurface (the surface depth itself)
enum { kTsdfExpected = 0, kTsdfInverse = 1, kTsdfSurface = 2 };
struct TsdfRule { double alpha_min, trunc, near, max_depth; float max_weight; int inverse; };

// block -> the node of this thread; false outside the grid
__device__ __forceinline__ bool node_of_thread(const TsdfVolume &vol, int &i, int &j, int &k) {
  const unsigned bxn = (unsigned)(vol.nx + kTX - 1) / kTX, byn = (unsigned)(vol.ny + kTY - 1) / kTY;
  unsigned b = blockIdx.x;
  const unsigned bx = b % bxn;
  b /= bxn;
  const unsigned by = b % byn;
  k = (int)(b / byn);
  i = (int)(bx * kTX + threadIdx.x);
  j = (int)(by * kTY + threadIdx.y);
  return i < vol.nx && j < vol.ny && k < vol.nz;
}

template <bool kColor>
__global__ __launch_bounds__(kTX * kTY) void tsdf_integrate_kernel(TsdfVolume vol, TsdfRule rule, TsdfBatch batch,
                                                                  const float *__restrict__ depth,
                                                                  const float *__restrict__ T,
                                                                  const float *__restrict__ image, int H, int W,
                                                                  float *__restrict__ tsdf, float *__restrict__ weight,
                                                                  float *__restrict__ color) {
  int i, j, k;
  if (!node_of_thread(vol, i, j, k)) return;
  const size_t n = ((size_t)k * vol.ny + j) * vol.nx + i;
  const double px = vol.ox + vol.voxel * (double)i, py = vol.oy + vol.voxel * (double)j, pz = vol.oz + vol.voxel * (double)k;
  float f = tsdf[n], w = weight[n], c[3] = {0.0f, 0.0f, 0.0f};
  if constexpr (kColor) { c[0] = color[n * 3]; c[1] = color[n * 3 + 1]; c[2] = color[n * 3 + 2]; }
  bool touched = false;
  const size_t P = (size_t)H * W;
  for (int v = 0; v < batch.n; ++v) {
    const TsdfView &cam = batch.v[v];
    const double z = (((double)cam.m[8] * px + (double)cam.m[9] * py) + (double)cam.m[10] * pz) + (double)cam.m[11];
    if (!(z > rule.near)) continue;
    const double xc = (((double)cam.m[0] * px + (double)cam.m[1] * py) + (double)cam.m[2] * pz) + (double)cam.m[3];
    const double yc = (((double)cam.m[4] * px + (double)cam.m[5] * py) + (double)cam.m[6] * pz) + (double)cam.m[7];
    const double fu = floor(((double)cam.fx * xc / z + (double)cam.cx) + 0.5);
    const double fv = floor(((double)cam.fy * yc / z + (double)cam.cy) + 0.5);
    if (!(fu >= 0.0 && fu < (double)W && fv >= 0.0 && fv < (double)H)) continue;
    const size_t pix = (size_t)v * P + (size_t)((int)fv) * W + (size_t)((int)fu);
    const double d = (double)depth[pix];
    double surf;
    if (rule.inverse == kTsdfSurface) {  // (T may be null: no opacity gate)
      if (!(d > 0.0 && d < HUGE_VAL)) continue;
      if (T != nullptr && !(1.0 - (double)T[pix] >= rule.alpha_min)) continue;
      surf = d;
    } else {
      const double A = 1.0 - (double)T[pix];
      if (!(A >= rule.alpha_min && A < HUGE_VAL && d > 0.0 && d < HUGE_VAL)) continue;
      surf = rule.inverse ? A / d : d / A;
    }
    if (rule.max_depth > 0.0 && surf > rule.max_depth) continue;
    const double s = surf - z;
    if (!(s >= -rule.trunc)) continue;
    const double val = fmin(1.0, s / rule.trunc);
    const double wd = (double)w, wn = wd + 1.0;
    f = (float)((wd * (double)f + val) / wn);
    if constexpr (kColor) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[ch] = (float)((wd * (double)c[ch] + (double)image[pix * 3 + ch]) / wn);
    }
    w = (float)wn;
    if (rule.max_weight > 0.0f && w > rule.max_weight) w = rule.max_weight;
    touched = true;
  }
  if (!touched) return;
  tsdf[n] = f;
  weight[n] = w;
  if constexpr (kColor) { color[n * 3] = c[0]; color[n * 3 + 1] = c[1]; color[n * 3 + 2] = c[2]; }
}

// ---------------------------------------------------------------------------------------------------------------------
// marching tetrahedra

// edge types in vertex order: the three axes, the three face diagonals, the body diagonal -> direction bits (x=1,y=2,z=4)
__device__ __forceinline__ int edge_type_of_dir(int d) {  // d in 1..7
  // d:      1  2  3  4  5  6  7
  // type:   0  1  3  2  4  5  6
  return (0x6542310 >> (4 * (d - 1))) & 7;
}
__device__ __forceinline__ int dir_of_edge_type(int e) {  // inverse of the above
  // type:   0  1  2  3  4  5  6
  // d:      1  2  4  3  5  6  7
  return (0x7653421 >> (4 * e)) & 7;
}

// The 16 cases of one tetrahedron with local corners 0..3 of POSITIVE orientation (det [v1-v0, v2-v0, v3-v0] > 0); bit c
// of the case = corner c inside.  A local edge (p, q), p < q, is coded p << 2 | q.  One inside corner i with the others
// (o0, o1, o2) such that (i, o0, o1, o2) is an even permutation: the triangle (i-o0, i-o1, i-o2), whose normal points away
// from i.  One outside corner: the same triangle about it, reversed.  Two inside (i0, i1), (i0, i1, o0, o1) even: the
// quadrilateral q0..q3 = (i0-o0, i0-o1, i1-o1, i1-o0) as the triangles (q0, q1, q2) and (q0, q2, q3).
struct TetTable { unsigned char n[16]; unsigned char e[16][6]; };

__host__ __device__ constexpr bool perm_odd(int a, int b, int c, int d) {
  const int p[4] = {a, b, c, d};
  int inv = 0;
  for (int x = 0; x < 4; ++x)
    for (int y = x + 1; y < 4; ++y) inv += p[x] > p[y];
  return inv & 1;
}
__host__ __device__ constexpr unsigned char edge_code(int p, int q) {
  return (unsigned char)(p < q ? (p << 2 | q) : (q << 2 | p));
}
__host__ __device__ constexpr TetTable make_tet_table() {
  TetTable t{};
  for (int m = 0; m < 16; ++m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int c = 0; c < 4; ++c) {
      if (m >> c & 1) in[ni++] = c;
      else out[no++] = c;
    }
    for (int x = 0; x < 6; ++x) t.e[m][x] = 0xFF;
    t.n[m] = 0;
    if (ni == 1) {
      int o1 = out[1], o2 = out[2];
      if (perm_odd(in[0], out[0], o1, o2)) { const int s = o1; o1 = o2; o2 = s; }
      t.e[m][0] = edge_code(in[0], out[0]); t.e[m][1] = edge_code(in[0], o1); t.e[m][2] = edge_code(in[0], o2);
      t.n[m] = 1;
    } else if (ni == 3) {
      int i1 = in[1], i2 = in[2];
      if (perm_odd(out[0], in[0], i1, i2)) { const int s = i1; i1 = i2; i2 = s; }
      t.e[m][0] = edge_code(out[0], in[0]); t.e[m][1] = edge_code(out[0], i2); t.e[m][2] = edge_code(out[0], i1);
      t.n[m] = 1;
    } else if (ni == 2) {
      int o0 = out[0], o1 = out[1];
      if (perm_odd(in[0], in[1], o0, o1)) { const int s = o0; o0 = o1; o1 = s; }
      const unsigned char q0 = edge_code(in[0], o0), q1 = edge_code(in[0], o1), q2 = edge_code(in[1], o1),
                          q3 = edge_code(in[1], o0);
      t.e[m][0] = q0; t.e[m][1] = q1; t.e[m][2] = q2; t.e[m][3] = q0; t.e[m][4] = q2; t.e[m][5] = q3;
      t.n[m] = 2;
    }
  }
  return t;
}
__device__ const TetTable kTet = make_tet_table();

// the six tetrahedra in the lexicographic order of (a, b, c): cube corners (0, a, a|b, 7), and whether (a, b, c) is an odd
// permutation of (x, y, z) -- then det [e_a, e_b, e_c] < 0 and every triangle of the table is reversed
__device__ __forceinline__ void tet_corners(int t, int (&corner)[4], bool &odd) {
  // t:   0 xyz  1 xzy  2 yxz  3 yzx  4 zxy  5 zyx
  const int a = (0x442211 >> (4 * t)) & 7, ab = (0x656353 >> (4 * t)) & 7;
  corner[0] = 0; corner[1] = a; corner[2] = ab; corner[3] = 7;
  odd = (0x26 >> t) & 1;  // t = 1, 2, 5
}

__device__ __forceinline__ int tet_triangles(int m) { return m == 0 || m == 15 ? 0 : (__popc(m) == 2 ? 2 : 1); }

struct Grid { int nx, ny, nz; };
__device__ __forceinline__ size_t node_offset(const Grid &g, int corner) {
  return (size_t)(corner & 1) + (size_t)((corner >> 1) & 1) * g.nx + (size_t)((corner >> 2) & 1) * g.nx * (size_t)g.ny;
}

// per node n, as the low corner of a cell: cell_ok (all eight nodes observed) and the cell's number of triangles
__global__ __launch_bounds__(kTX * kTY) void tsdf_mark_cells_kernel(TsdfVolume vol, const float *__restrict__ tsdf,
                                                                   const float *__restrict__ weight, float min_weight,
                                                                   unsigned char *__restrict__ cell_ok,
                                                                   int *__restrict__ tri_count) {
  int i, j, k;
  if (!node_of_thread(vol, i, j, k)) return;
  const Grid g = {vol.nx, vol.ny, vol.nz};
  const size_t n = ((size_t)k * g.ny + j) * g.nx + i;
  bool ok = i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz;
  int inside = 0, tris = 0;
  if (ok) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const size_t q = n + node_offset(g, c);
      ok = ok && weight[q] >= min_weight;
      inside |= (tsdf[q] < 0.0f ? 1 : 0) << c;
    }
  }
  if (ok && inside != 0 && inside != 255) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      int corner[4];
      bool odd;
      tet_corners(t, corner, odd);
      int m = 0;
#pragma unroll
      for (int l = 0; l < 4; ++l) m |= ((inside >> corner[l]) & 1) << l;
      tris += tet_triangles(m);
    }
  }
  cell_ok[n] = ok ? 1 : 0;
  tri_count[n] = tris;
}

// per node n, as the lower end of its seven edges: the mask of the edges that carry a vertex (a sign change, and at least
// one meshed cell around the edge) and their number
__global__ __launch_bounds__(kTX * kTY) void tsdf_mark_edges_kernel(TsdfVolume vol, const float *__restrict__ tsdf,
                                                                   const unsigned char *__restrict__ cell_ok,
                                                                   unsigned char *__restrict__ edge_mask,
                                                                   int *__restrict__ vert_count) {
  int i, j, k;
  if (!node_of_thread(vol, i, j, k)) return;
  const Grid g = {vol.nx, vol.ny, vol.nz};
  const size_t n = ((size_t)k * g.ny + j) * g.nx + i;
  const bool in_a = tsdf[n] < 0.0f;
  int mask = 0;
#pragma unroll
  for (int d = 1; d < 8; ++d) {
    if (i + (d & 1) >= g.nx || j + ((d >> 1) & 1) >= g.ny || k + ((d >> 2) & 1) >= g.nz) continue;
    if ((tsdf[n + node_offset(g, d)] < 0.0f) == in_a) continue;
    // the cells that hold both ends: low corner n - s for every subset s of the axes the edge does not move along
    const int free_axes = ~d & 7;
    bool used = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if ((s & free_axes) != s) continue;
      if (((s & 1) && i == 0) || ((s & 2) && j == 0) || ((s & 4) && k == 0)) continue;
      used = used || cell_ok[n - node_offset(g, s)] != 0;
    }
    if (used) mask |= 1 << edge_type_of_dir(d);
  }
  edge_mask[n] = (unsigned char)mask;
  vert_count[n] = __popc(mask);
}

template <bool kColor>
__global__ __launch_bounds__(kTX * kTY) void tsdf_emit_kernel(TsdfVolume vol, const float *__restrict__ tsdf,
                                                             const float *__restrict__ color,
                                                             const unsigned char *__restrict__ cell_ok,
                                                             const unsigned char *__restrict__ edge_mask,
                                                             const long long *__restrict__ vert_offset,
                                                             const long long *__restrict__ tri_offset,
                                                             long long num_vertices, long long num_faces,
                                                             float *__restrict__ vertices, float *__restrict__ vcolors,
                                                             int *__restrict__ faces) {
  int i, j, k;
  if (!node_of_thread(vol, i, j, k)) return;
  const Grid g = {vol.nx, vol.ny, vol.nz};
  const size_t n = ((size_t)k * g.ny + j) * g.nx + i;
  const int mask = edge_mask[n];
  if (mask) {
    const double pa[3] = {vol.ox + vol.voxel * (double)i, vol.oy + vol.voxel * (double)j, vol.oz + vol.voxel * (double)k};
    const double fa = (double)tsdf[n];
    long long out = vert_offset[n];
    for (int e = 0; e < 7; ++e) {
      if (!((mask >> e) & 1)) continue;
      const int d = dir_of_edge_type(e);
      const size_t q = n + node_offset(g, d);
      const double fb = (double)tsdf[q];
      const double t = fa / (fa - fb);
      if (out >= 0 && out < num_vertices) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          const int ib = (ax == 0 ? i : ax == 1 ? j : k) + ((d >> ax) & 1);
          const double pb = (ax == 0 ? vol.ox : ax == 1 ? vol.oy : vol.oz) + vol.voxel * (double)ib;
          vertices[out * 3 + ax] = (float)(pa[ax] + t * (pb - pa[ax]));
        }
        if constexpr (kColor) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const double ca = (double)color[n * 3 + ch], cb = (double)color[q * 3 + ch];
            vcolors[out * 3 + ch] = (float)(ca + t * (cb - ca));
          }
        }
      }
      ++out;
    }
  }
  if (!cell_ok[n]) return;
  int inside = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) inside |= (tsdf[n + node_offset(g, c)] < 0.0f ? 1 : 0) << c;
  if (inside == 0 || inside == 255) return;
  long long out = tri_offset[n];
  for (int t = 0; t < 6; ++t) {
    int corner[4];
    bool odd;
    tet_corners(t, corner, odd);
    int m = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) m |= ((inside >> corner[l]) & 1) << l;
    const int nt = kTet.n[m];
    for (int tri = 0; tri < nt; ++tri) {
      int idx[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const int code = kTet.e[m][tri * 3 + x];
        const int cp = corner[code >> 2], cq = corner[code & 3];  // cp is a subset of cq: the lower end
        const size_t lower = n + node_offset(g, cp);
        const int e = edge_type_of_dir(cp ^ cq);
        idx[x] = (int)(vert_offset[lower] + __popc((int)edge_mask[lower] & ((1 << e) - 1)));
      }
      if (out >= 0 && out < num_faces) {
        faces[out * 3] = idx[0];
        faces[out * 3 + 1] = odd ? idx[2] : idx[1];
        faces[out * 3 + 2] = odd ? idx[1] : idx[2];
      }
      ++out;
    }
  }
}

// the checks every entry point makes on the grid; `fn`: the public function that was called
int check_grid(const char *fn, int nx, int ny, int nz, float voxel) {
  GS_REQUIRE_IN(fn, nx > 0 && ny > 0 && nz > 0, "the grid size must be positive");
  GS_REQUIRE_IN(fn, (long long)nx * ny <= GSPLAT_TSDF_MAX_NODES && (long long)nx * ny * nz <= GSPLAT_TSDF_MAX_NODES,
                "the grid has more than GSPLAT_TSDF_MAX_NODES nodes");
  GS_REQUIRE_IN(fn, std::isfinite(voxel) && voxel > 0.0f, "voxel must be finite and positive");
  return GSPLAT_OK;
}

unsigned int grid_blocks(int nx, int ny, int nz) {
  return (unsigned int)((long long)gs::div_up(nx, kTX) * gs::div_up(ny, kTY) * nz);  // <= the node count
}

// gsplat_tsdf_integrate (mode kTsdfExpected / kTsdfInverse) and gsplat_tsdf_integrate_surface (kTsdfSurface, T may be null)
int integrate(const char *fn, float *tsdf, float *weight, float *color, int nx, int ny, int nz, const float *origin,
              float voxel, const float *depth, const float *T, const float *image, const float *view,
              const float *intrinsics, int num_views, int rows, int cols, int mode, float alpha_min, float trunc, float near,
              float max_depth, float max_weight, void *stream) {
  if (int rc = check_grid(fn, nx, ny, nz, voxel)) return rc;
  GS_REQUIRE_IN(fn, rows > 0 && cols > 0 && num_views >= 0, "image size must be positive, num_views not negative");
  GS_REQUIRE_IN(fn, std::isfinite(trunc) && trunc > 0.0f, "trunc must be finite and positive");
  GS_REQUIRE_IN(fn, alpha_min > 0.0f && alpha_min <= 1.0f, "alpha_min must lie in (0, 1]");
  GS_REQUIRE_IN(fn, (image != nullptr) == (color != nullptr), "image and color go together");
  if (num_views == 0) return GSPLAT_OK;
  GS_REQUIRE_IN(fn, tsdf && weight && origin && depth && (T || mode == kTsdfSurface) && view && intrinsics,
                "a required pointer is NULL");
  for (int v = 0; v < num_views; ++v) {
    const float *k = intrinsics + 4 * v;
    GS_REQUIRE_IN(fn, std::isfinite(k[0]) && std::isfinite(k[1]) && std::isfinite(k[2]) && std::isfinite(k[3]),
               "the intrinsics must be finite");
    GS_REQUIRE_IN(fn, k[0] != 0.0f && k[1] != 0.0f, "fx and fy must not be 0");
  }
  GS_REQUIRE_DEV_IN(fn, tsdf); GS_REQUIRE_DEV_IN(fn, weight); GS_REQUIRE_DEV_IN(fn, depth);
  if (T) GS_REQUIRE_DEV_IN(fn, T);
  if (color) { GS_REQUIRE_DEV_IN(fn, color); GS_REQUIRE_DEV_IN(fn, image); }
  const TsdfVolume vol = {(double)origin[0], (double)origin[1], (double)origin[2], (double)voxel, nx, ny, nz};
  const TsdfRule rule = {(double)alpha_min, (double)trunc, (double)near, (double)max_depth, max_weight, mode};
  const dim3 block(kTX, kTY);
  const unsigned int blocks = grid_blocks(nx, ny, nz);
  const size_t P = (size_t)rows * cols;
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < num_views; base += kTsdfViews) {
    TsdfBatch batch;
    batch.n = std::min(kTsdfViews, num_views - base);
    for (int v = 0; v < kTsdfViews; ++v) {
      const int src = base + std::min(v, batch.n - 1);  // (the unused slots repeat the last view: no uninitialised bytes)
      std::memcpy(batch.v[v].m, view + 12 * (size_t)src, 12 * sizeof(float));
      const float *k = intrinsics + 4 * (size_t)src;
      batch.v[v].fx = k[0]; batch.v[v].fy = k[1]; batch.v[v].cx = k[2]; batch.v[v].cy = k[3];
    }
    const float *d = depth + base * P, *t = T ? T + base * P : nullptr;
    if (color)
      tsdf_integrate_kernel<true><<<blocks, block, 0, st>>>(vol, rule, batch, d, t, image + base * P * 3, rows, cols, tsdf,
                                                            weight, color);
    else
      tsdf_integrate_kernel<false><<<blocks, block, 0, st>>>(vol, rule, batch, d, t, nullptr, rows, cols, tsdf, weight,
                                                             nullptr);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

}  // namespace

extern "C" {

int gsplat_tsdf_integrate(float *tsdf, float *weight, float *color, int nx, int ny, int nz, const float *origin, float voxel,
                          const float *depth, const float *T, const float *image, const float *view,
                          const float *intrinsics, int num_views, int rows, int cols, int inverse, float alpha_min,
                          float trunc, float near, float max_depth, float max_weight, void *stream) {
  return integrate(__func__, tsdf, weight, color, nx, ny, nz, origin, voxel, depth, T, image, view, intrinsics, num_views,
                   rows, cols, inverse != 0 ? kTsdfInverse : kTsdfExpected, alpha_min, trunc, near, max_depth, max_weight,
                   stream);
}

int gsplat_tsdf_integrate_surface(float *tsdf, float *weight, float *color, int nx, int ny, int nz, const float *origin,
                                  float voxel, const float *depth, const float *T, const float *image, const float *view,
                                  const float *intrinsics, int num_views, int rows, int cols, float alpha_min, float trunc,
                                  float near, float max_depth, float max_weight, void *stream) {
  return integrate(__func__, tsdf, weight, color, nx, ny, nz, origin, voxel, depth, T, image, view, intrinsics, num_views,
                   rows, cols, kTsdfSurface, alpha_min, trunc, near, max_depth, max_weight, stream);
}

int gsplat_tsdf_views_per_pass(void) { return kTsdfViews; }

int gsplat_tsdf_mark(const float *tsdf, const float *weight, int nx, int ny, int nz, float min_weight,
                     unsigned char *cell_ok, int *tri_count, unsigned char *edge_mask, int *vert_count, void *stream) {
  if (int rc = check_grid(__func__, nx, ny, nz, 1.0f)) return rc;
  GS_REQUIRE(!std::isnan(min_weight), "min_weight must be a number");
  GS_REQUIRE(tsdf && weight && cell_ok && tri_count && edge_mask && vert_count, "a required pointer is NULL");
  GS_REQUIRE_DEV(tsdf); GS_REQUIRE_DEV(weight); GS_REQUIRE_DEV(cell_ok); GS_REQUIRE_DEV(tri_count);
  GS_REQUIRE_DEV(edge_mask); GS_REQUIRE_DEV(vert_count);
  const TsdfVolume vol = {0.0, 0.0, 0.0, 1.0, nx, ny, nz};
  const dim3 block(kTX, kTY);
  const unsigned int blocks = grid_blocks(nx, ny, nz);
  hipStream_t st = (hipStream_t)stream;
  tsdf_mark_cells_kernel<<<blocks, block, 0, st>>>(vol, tsdf, weight, min_weight, cell_ok, tri_count);
  GS_LAUNCH_CHECK();
  tsdf_mark_edges_kernel<<<blocks, block, 0, st>>>(vol, tsdf, cell_ok, edge_mask, vert_count);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_tsdf_emit(const float *tsdf, const float *color, int nx, int ny, int nz, const float *origin, float voxel,
                     const unsigned char *cell_ok, const unsigned char *edge_mask, const long long *vert_offset,
                     const long long *tri_offset, long long num_vertices, long long num_faces, float *vertices,
                     float *vertex_colors, int *faces, void *stream) {
  if (int rc = check_grid(__func__, nx, ny, nz, voxel)) return rc;
  GS_REQUIRE(num_vertices >= 0 && num_faces >= 0 && num_vertices <= 0x7FFFFFFFll && num_faces <= 0x7FFFFFFFll,
             "the vertex and face counts must lie in 0 .. 2^31 - 1");
  GS_REQUIRE((color != nullptr) == (vertex_colors != nullptr) || num_vertices == 0, "color and vertex_colors go together");
  if (num_vertices == 0 && num_faces == 0) return GSPLAT_OK;
  GS_REQUIRE(tsdf && origin && cell_ok && edge_mask && vert_offset && tri_offset, "a required pointer is NULL");
  GS_REQUIRE(num_vertices == 0 || vertices, "vertices is NULL");
  GS_REQUIRE(num_faces == 0 || faces, "faces is NULL");
  GS_REQUIRE_DEV(tsdf); GS_REQUIRE_DEV(cell_ok); GS_REQUIRE_DEV(edge_mask); GS_REQUIRE_DEV(vert_offset);
  GS_REQUIRE_DEV(tri_offset);
  if (vertices) GS_REQUIRE_DEV(vertices);
  if (faces) GS_REQUIRE_DEV(faces);
  if (color) { GS_REQUIRE_DEV(color); GS_REQUIRE_DEV(vertex_colors); }
  const TsdfVolume vol = {(double)origin[0], (double)origin[1], (double)origin[2], (double)voxel, nx, ny, nz};
  const dim3 block(kTX, kTY);
  const unsigned int blocks = grid_blocks(nx, ny, nz);
  hipStream_t st = (hipStream_t)stream;
  if (color && vertex_colors)
    tsdf_emit_kernel<true><<<blocks, block, 0, st>>>(vol, tsdf, color, cell_ok, edge_mask, vert_offset, tri_offset,
                                                     num_vertices, num_faces, vertices, vertex_colors, faces);
  else
    tsdf_emit_kernel<false><<<blocks, block, 0, st>>>(vol, tsdf, nullptr, cell_ok, edge_mask, vert_offset, tri_offset,
                                                      num_vertices, num_faces, vertices, nullptr, faces);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // extern "C"
