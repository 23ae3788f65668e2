// gs_bilagrid.hip -- per-view appearance compensation with a bilateral grid ("Bilateral Guided Radiance Field Processing",
// Wang et al. 2024): gsplat_bilagrid_slice maps a render to a corrected image through a [12, L, Hg, Wg] grid of 3x4 colour
// affines, gsplat_bilagrid_slice_backward takes dL/d corrected back to dL/d render and dL/d grid, and
// gsplat_bilagrid_tv_loss is the grid's total-variation regulariser; definitions: include/gsplat_hip.h.
//
// Like the other image-space terms (gs_regloss.h) everything is evaluated in double from the float inputs and every
// stored value is rounded to float once.  The slice, dL/d render and the TV loss are per-pixel (per-element) maps and
// fixed-order sums.  dL/d grid is a reduction with heavy fan-in -- at 1920 x 1080 under a 16 x 16 x 8 grid each value is
// the sum of some 37 000 pixels -- and is formed WITHOUT atomics, in two passes over a slab of partial sums:
//   1. grid_partial_kernel: one workgroup per 32 x 32 pixel tile stages the tile in LDS (render, dL/d corrected, the
//      x-cell of every column, the y-cell of every row), its pixels ordered by their z-cell with a counting sort whose
//      order is a function of the data alone.  A tile touches a small rectangle of xy vertices (3 x 3 at most in the case
//      above) x L levels x 12 coefficients; (vertex, level, row of the 3x4 matrix) = four coefficients belong to a group
//      of 1 .. 64 lanes, which walks the pixels of the two z-cells that reach the level in slot order, adds those that
//      reach the vertex, and stores the four sums in the tile's slots of the slab (doubles).  Every slot is written, zeros
//      included.
//   2. grid_finish_kernel: a group of 1 .. 64 lanes per grid value sums the slots of the tiles that touch its vertex, in
//      tile order and then through a fixed butterfly, rounds to float once and stores or adds.
// No pixel is read twice, no adder shares a destination: two runs give the same bits for every output, dL/d grid included.
#include <cmath>

#include "gs_common.h"
#include "gs_regloss.h"

namespace {

constexpr int kMaxGridXY = 64, kMaxGridL = 16;
constexpr int kTile = 32, kTilePixels = kTile * kTile;  // pass 1's pixel tile
constexpr double kLumaR = 0.299, kLumaG = 0.587, kLumaB = 0.114;

struct Grid {
  const float *v;  // [12, L, Hg, Wg]
  int Wg, Hg, L;
};

// the cell of coordinate c >= 0 on an axis of n vertices: the two vertices and the weight of the second
struct Cell {
  int i0, i1;
  double t;
};
__host__ __device__ inline Cell cell_of(double c, int n) {
  const int lim = n >= 2 ? n - 2 : 0;
  int i0 = (int)floor(c);
  if (i0 > lim) i0 = lim;
  if (i0 < 0) i0 = 0;
  Cell r;
  r.i0 = i0;
  r.i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  r.t = c - (double)i0;
  return r;
}
// the grid coordinate of pixel centre x on an image axis of `size` pixels and a grid axis of n vertices
__host__ __device__ inline double grid_coord(int x, int size, int n) {
  return ((double)x + 0.5) / (double)size * (double)(n - 1);
}
__device__ __forceinline__ double guidance_of(float r0, float r1, float r2) {
  return (kLumaR * (double)r0 + kLumaG * (double)r1) + kLumaB * (double)r2;
}
// the z coordinate of a guidance value: clamped to [0, 1] (a NaN counts as 0: no index leaves the grid)
__device__ __forceinline__ double z_coord(double g, int L) {
  const double c = g > 0.0 ? (g < 1.0 ? g : 1.0) : 0.0;
  return c * (double)(L - 1);
}
// what a pixel in cell (c.i0, c.i1, c.t) adds to vertex i: (1 - t) at i0 plus t at i1 (one vertex when the axis has one)
__device__ __forceinline__ double weight_at(int i, int i0, int i1, double t) {
  return (i == i0 ? 1.0 - t : 0.0) + (i == i1 ? t : 0.0);
}

// The 12 interpolated coefficients A of a pixel and, with kSlope, dA / d gz: the difference of the cell's two z-levels,
// bilinear in xy.
template <bool kSlope>
__device__ __forceinline__ void coefficients(const Grid &g, const Cell &cx, const Cell &cy, const Cell &cz, double (&A)[12],
                                             double (&dA)[12]) {
  const double w00 = (1.0 - cx.t) * (1.0 - cy.t), w01 = cx.t * (1.0 - cy.t), w10 = (1.0 - cx.t) * cy.t, w11 = cx.t * cy.t;
  const size_t level = (size_t)g.Hg * g.Wg;
  const size_t o00 = (size_t)cy.i0 * g.Wg + cx.i0, o01 = (size_t)cy.i0 * g.Wg + cx.i1;
  const size_t o10 = (size_t)cy.i1 * g.Wg + cx.i0, o11 = (size_t)cy.i1 * g.Wg + cx.i1;
#pragma unroll
  for (int ch = 0; ch < 12; ++ch) {
    const float *lo = g.v + ((size_t)ch * g.L + cz.i0) * level, *hi = g.v + ((size_t)ch * g.L + cz.i1) * level;
    const double a00 = lo[o00], a01 = lo[o01], a10 = lo[o10], a11 = lo[o11];
    const double b00 = hi[o00], b01 = hi[o01], b10 = hi[o10], b11 = hi[o11];
    const double za = 1.0 - cz.t, zb = cz.t;
    A[ch] = (((w00 * za) * a00 + (w01 * za) * a01) + ((w10 * za) * a10 + (w11 * za) * a11)) +
            (((w00 * zb) * b00 + (w01 * zb) * b01) + ((w10 * zb) * b10 + (w11 * zb) * b11));
    if constexpr (kSlope)
      dA[ch] = (w00 * (b00 - a00) + w01 * (b01 - a01)) + (w10 * (b10 - a10) + w11 * (b11 - a11));
  }
}

struct SliceArgs {
  Grid grid;
  const float *image;     // [H, W, 3]
  const float *grad_out;  // [H, W, 3] (backward)
  float *out;             // the corrected image (forward) or dL/d image (backward)
  int H, W;
};

// one pixel per thread; kBackward: out = dL/d image
template <bool kBackward>
__global__ __launch_bounds__(256) void slice_kernel(SliceArgs a) {
  const long long P = (long long)a.H * a.W;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
    const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
    const size_t at = (size_t)p * 3;
    const float r0 = a.image[at], r1 = a.image[at + 1], r2 = a.image[at + 2];
    const double g = guidance_of(r0, r1, r2);
    const Cell cx = cell_of(grid_coord(x, a.W, a.grid.Wg), a.grid.Wg), cy = cell_of(grid_coord(y, a.H, a.grid.Hg), a.grid.Hg);
    const Cell cz = cell_of(z_coord(g, a.grid.L), a.grid.L);
    double A[12], dA[12];
    if constexpr (!kBackward) {
      coefficients<false>(a.grid, cx, cy, cz, A, dA);
#pragma unroll
      for (int r = 0; r < 3; ++r)
        a.out[at + r] = (float)(((A[r * 4] * (double)r0 + A[r * 4 + 1] * (double)r1) + A[r * 4 + 2] * (double)r2) + A[r * 4 + 3]);
    } else {
      const double G0 = a.grad_out[at], G1 = a.grad_out[at + 1], G2 = a.grad_out[at + 2];
      // the guidance moves the z coordinate only strictly inside (0, 1) -- at the two ends themselves the gradient is 0,
      // as grid_sample's border padding has it -- and only when there is a z axis
      const bool slope = a.grid.L > 1 && g > 0.0 && g < 1.0;
      double through_z = 0.0;
      if (slope) {
        coefficients<true>(a.grid, cx, cy, cz, A, dA);
        const double G[3] = {G0, G1, G2};
#pragma unroll
        for (int r = 0; r < 3; ++r)
          through_z += G[r] * (((dA[r * 4] * (double)r0 + dA[r * 4 + 1] * (double)r1) + dA[r * 4 + 2] * (double)r2) + dA[r * 4 + 3]);
        through_z *= (double)(a.grid.L - 1);
      } else {
        coefficients<false>(a.grid, cx, cy, cz, A, dA);
      }
      const double luma[3] = {kLumaR, kLumaG, kLumaB};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double direct = (A[c] * G0 + A[4 + c] * G1) + A[8 + c] * G2;
        a.out[at + c] = (float)(slope ? direct + through_z * luma[c] : direct);
      }
    }
  }
}

// ---------------------------------------------------------------- dL/d grid: the slab of per-tile partial sums

// the xy vertices a run of pixels [first, last] of an axis touches: the first pixel's i0 .. the last pixel's i1
__host__ __device__ inline void vertex_range(int first, int last, int size, int n, int &lo, int &hi) {
  lo = cell_of(grid_coord(first, size, n), n).i0;
  hi = cell_of(grid_coord(last, size, n), n).i1;
}
__host__ __device__ inline void tile_vertex_range(int tile, int size, int n, int &lo, int &hi) {
  const int first = tile * kTile, last = (first + kTile < size ? first + kTile : size) - 1;
  vertex_range(first, last, size, n, lo, hi);
}

struct SlabArgs {
  Grid grid;
  const float *image, *grad_out;
  int H, W;
  int ntx, nty;    // pixel tiles
  int ni_s, nj_s;  // the slots of a tile: the largest vertex rectangle any tile touches
  int lanes;       // pass 2: lanes per grid value, a power of two <= 64
  int add;
  double *slab;    // [nty * ntx][nj_s][ni_s][L][12]
  float *grad_grid;
};

__global__ __launch_bounds__(256) void grid_partial_kernel(SlabArgs a) {
  // the tile's pixels, ordered by their z-cell (a counting sort; inside a cell by pixel index): slot q holds dL/d out, the
  // colour, the weight of the cell's upper level and the pixel's column and row in the tile
  __shared__ float s_g[kTilePixels * 3], s_r[kTilePixels * 3];
  __shared__ double s_tz[kTilePixels];
  __shared__ unsigned char s_lx[kTilePixels], s_ly[kTilePixels];
  __shared__ double s_tx[kTile], s_ty[kTile];
  __shared__ int s_i0[kTile], s_j0[kTile];
  __shared__ int s_count[16][kMaxGridL];  // [trip x 4 + wave][z-cell]: the pixels of a wave's trip, then their first slot
  __shared__ int s_start[kMaxGridL + 1];  // the first slot of a z-cell
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, Wg = a.grid.Wg, Hg = a.grid.Hg, L = a.grid.L;
  const int tx = (int)(blockIdx.x % (unsigned)a.ntx), ty = (int)(blockIdx.x / (unsigned)a.ntx);
  const int x0 = tx * kTile, y0 = ty * kTile;
  const int ncols = min(kTile, a.W - x0), nrows = min(kTile, a.H - y0);
  if (tid < kTile) {
    if (tid < ncols) {
      const Cell c = cell_of(grid_coord(x0 + tid, a.W, Wg), Wg);
      s_i0[tid] = c.i0; s_tx[tid] = c.t;
    }
  } else if (tid < 2 * kTile) {
    const int l = tid - kTile;
    if (l < nrows) {
      const Cell c = cell_of(grid_coord(y0 + l, a.H, Hg), Hg);
      s_j0[l] = c.i0; s_ty[l] = c.t;
    }
  }
  // a thread's four pixels (one per trip) stay in registers until their slots are known
  float r[4][3], g[4][3];
  double tz[4];
  int k0[4], rank[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int p = m * 256 + tid, lx = p % kTile, ly = p / kTile;
    k0[m] = -1;
    if (lx < ncols && ly < nrows) {
      const size_t at = ((size_t)(y0 + ly) * a.W + (x0 + lx)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) { r[m][c] = a.image[at + c]; g[m][c] = a.grad_out[at + c]; }
      const Cell cz = cell_of(z_coord(guidance_of(r[m][0], r[m][1], r[m][2]), L), L);
      k0[m] = cz.i0; tz[m] = cz.t;
    }
    rank[m] = 0;
    for (int k = 0; k < L; ++k) {  // (every lane of the wave: the ballots are wave-wide)
      const unsigned long long mask = __ballot(k0[m] == k);
      if (k0[m] == k) rank[m] = __popcll(mask & ((1ull << lane) - 1ull));
      if (lane == 0) s_count[m * 4 + wave][k] = __popcll(mask);
    }
  }
  __syncthreads();
  if (tid < L) {  // a z-cell's pixels of the trips and waves in front: the same order in every run
    int sum = 0;
    for (int t = 0; t < 16; ++t) { const int n = s_count[t][tid]; s_count[t][tid] = sum; sum += n; }
    s_start[tid + 1] = sum;  // (the cell's size, for now)
  }
  __syncthreads();
  if (tid == 0) {
    s_start[0] = 0;
    for (int k = 0; k < L; ++k) s_start[k + 1] += s_start[k];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (k0[m] < 0) continue;
    const int p = m * 256 + tid, q = s_start[k0[m]] + s_count[m * 4 + wave][k0[m]] + rank[m];
#pragma unroll
    for (int c = 0; c < 3; ++c) { s_r[q * 3 + c] = r[m][c]; s_g[q * 3 + c] = g[m][c]; }
    s_tz[q] = tz[m];
    s_lx[q] = (unsigned char)(p % kTile); s_ly[q] = (unsigned char)(p / kTile);
  }
  __syncthreads();

  const int imin = s_i0[0], imax = min(s_i0[ncols - 1] + 1, Wg - 1);
  const int jmin = s_j0[0], jmax = min(s_j0[nrows - 1] + 1, Hg - 1);
  const int ni = imax - imin + 1, nj = jmax - jmin + 1;
  const size_t slots = (size_t)a.ni_s * a.nj_s * L * 12;
  double *mine = a.slab + (size_t)blockIdx.x * slots;
  // (matrix row, vertex, level) = four coefficients belong to a group of S lanes: the lanes share the pixels of the two
  // z-cells that reach the level, each adds its own in slot order, and a fixed butterfly adds the lanes.  S is the largest
  // power of two with S x (rows x vertices) <= 256, whatever L: a group then takes the levels of its row and vertex one
  // after the other, and since every pixel lies in one z-cell all groups walk the same number of pixels -- a render,
  // whose tile sits in one or two z-cells, keeps every lane as busy as noise does
  const int nd = ni * nj * L * 3;
  int S = 1;
  while (S < 64 && 2 * S * (ni * nj * 3) <= 256) S *= 2;
  const int s = tid % S, groups = 256 / S;
  for (int d = tid / S; d < nd; d += groups) {
    const int row = d % 3, il = (d / 3) % ni, jl = (d / (3 * ni)) % nj, k = d / (3 * ni * nj);
    const int i = imin + il, j = jmin + jl;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    for (int b = max(k - 1, 0); b <= k; ++b) {  // the z-cells [b, b + 1] with k at one end
      const int b1 = min(b + 1, L - 1);
      for (int q = s_start[b] + s; q < s_start[b + 1]; q += S) {
        const int lx = s_lx[q], ly = s_ly[q];
        const int i0 = s_i0[lx], i1 = min(i0 + 1, Wg - 1), j0 = s_j0[ly], j1 = min(j0 + 1, Hg - 1);
        if ((i != i0 && i != i1) || (j != j0 && j != j1)) continue;
        const double w = (weight_at(i, i0, i1, s_tx[lx]) * weight_at(j, j0, j1, s_ty[ly])) * weight_at(k, b, b1, s_tz[q]);
        const double gw = w * (double)s_g[q * 3 + row];
        acc0 += gw * (double)s_r[q * 3];
        acc1 += gw * (double)s_r[q * 3 + 1];
        acc2 += gw * (double)s_r[q * 3 + 2];
        acc3 += gw;
      }
    }
    for (int off = S >> 1; off > 0; off >>= 1) {
      acc0 += __shfl_xor(acc0, off, 64); acc1 += __shfl_xor(acc1, off, 64);
      acc2 += __shfl_xor(acc2, off, 64); acc3 += __shfl_xor(acc3, off, 64);
    }
    if (s == 0 && il < a.ni_s && jl < a.nj_s) {  // (always: ni_s and nj_s are the largest ni and nj of any tile)
      double *dst = mine + (((size_t)jl * a.ni_s + il) * L + k) * 12 + row * 4;
      dst[0] = acc0; dst[1] = acc1; dst[2] = acc2; dst[3] = acc3;
    }
  }
}

// A group of a.lanes lanes per grid value: the tiles whose vertex rectangle holds the value's vertex, in tile order.
__global__ __launch_bounds__(256) void grid_finish_kernel(SlabArgs a) {
  // per x vertex (0 .. 63) and y vertex (64 .. 127): the first and last tile that touches it (first > last: none)
  __shared__ int s_first[2 * kMaxGridXY], s_last[2 * kMaxGridXY];
  const int tid = (int)threadIdx.x, Wg = a.grid.Wg, Hg = a.grid.Hg, L = a.grid.L;
  if (tid < 2 * kMaxGridXY) {
    const bool is_y = tid >= kMaxGridXY;
    const int v = is_y ? tid - kMaxGridXY : tid, n = is_y ? Hg : Wg, size = is_y ? a.H : a.W, nt = is_y ? a.nty : a.ntx;
    int first = nt, last = -1;
    if (v < n)
      for (int t = 0; t < nt; ++t) {
        int lo, hi;
        tile_vertex_range(t, size, n, lo, hi);
        if (v >= lo && v <= hi) { first = min(first, t); last = max(last, t); }
      }
    s_first[tid] = first; s_last[tid] = last;
  }
  __syncthreads();
  const long long n_values = 12ll * L * Hg * Wg;
  const long long e = ((long long)blockIdx.x * 256 + tid) / a.lanes;
  const int s = tid % a.lanes;
  const bool live = e < n_values;
  double sum = 0.0;
  if (live) {
    const int i = (int)(e % Wg), j = (int)((e / Wg) % Hg), k = (int)((e / ((long long)Wg * Hg)) % L);
    const int ch = (int)(e / ((long long)Wg * Hg * L));
    const int txa = s_first[i], tya = s_first[kMaxGridXY + j];
    const int nx = s_last[i] - txa + 1, ny = s_last[kMaxGridXY + j] - tya + 1;
    if (nx > 0 && ny > 0) {
      const size_t slots = (size_t)a.ni_s * a.nj_s * L * 12;
      for (int t = s; t < nx * ny; t += a.lanes) {
        const int tx = txa + t % nx, ty = tya + t / nx;
        int lo, hi;
        tile_vertex_range(tx, a.W, Wg, lo, hi);
        const int il = i - lo;
        tile_vertex_range(ty, a.H, Hg, lo, hi);
        const int jl = j - lo;
        if (il >= 0 && il < a.ni_s && jl >= 0 && jl < a.nj_s)
          sum += a.slab[((size_t)ty * a.ntx + tx) * slots + (((size_t)jl * a.ni_s + il) * L + k) * 12 + ch];
      }
    }
  }
  for (int off = a.lanes >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (live && s == 0) {
    const float v = (float)sum;
    a.grad_grid[e] = a.add ? a.grad_grid[e] + v : v;
  }
}

// ---------------------------------------------------------------- the TV loss

struct TvArgs {
  Grid grid;
  double cx, cy, cz;  // 1 / the pairs along the axis, 0 for an axis of one vertex
  double weight;
  int add;
  float *grad;      // or null
  double *partial;  // or null
};

__global__ __launch_bounds__(256) void tv_kernel(TvArgs a) {
  const int Wg = a.grid.Wg, Hg = a.grid.Hg, L = a.grid.L;
  const int n = 12 * L * Hg * Wg, sx = 1, sy = Wg, sz = Wg * Hg;
  double sum = 0.0;
  for (int e = (int)(blockIdx.x * 256 + threadIdx.x); e < n; e += (int)(gridDim.x * 256)) {
    const int i = e % Wg, j = (e / Wg) % Hg, k = (e / sz) % L;
    const double v = a.grid.v[e];
    double g = 0.0;
    // a pair's squared difference is counted at its lower element; its gradient at both
    if (i + 1 < Wg) { const double d = v - (double)a.grid.v[e + sx]; sum += a.cx * (d * d); g += (2.0 * a.cx) * d; }
    if (i > 0) g += (2.0 * a.cx) * (v - (double)a.grid.v[e - sx]);
    if (j + 1 < Hg) { const double d = v - (double)a.grid.v[e + sy]; sum += a.cy * (d * d); g += (2.0 * a.cy) * d; }
    if (j > 0) g += (2.0 * a.cy) * (v - (double)a.grid.v[e - sy]);
    if (k + 1 < L) { const double d = v - (double)a.grid.v[e + sz]; sum += a.cz * (d * d); g += (2.0 * a.cz) * d; }
    if (k > 0) g += (2.0 * a.cz) * (v - (double)a.grid.v[e - sz]);
    if (a.grad) {
      const float r = (float)(a.weight * g);
      a.grad[e] = a.add ? a.grad[e] + r : r;
    }
  }
  if (a.partial) gs::block_partial(sum, a.partial);
}

int check_grid(const char *fn, const float *grid, int grid_w, int grid_h, int grid_l) {
  GS_REQUIRE_IN(fn, grid_w >= 1 && grid_w <= kMaxGridXY && grid_h >= 1 && grid_h <= kMaxGridXY,
                "grid_w and grid_h must be 1 .. 64");
  GS_REQUIRE_IN(fn, grid_l >= 1 && grid_l <= kMaxGridL, "grid_l must be 1 .. 16");
  GS_REQUIRE_IN(fn, grid != nullptr, "grid is null");
  return GSPLAT_OK;
}

bool overlap(const void *a, const void *b, size_t bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p < q + bytes && q < p + bytes;
}

int pixel_blocks(long long P) { return (int)std::min<long long>(8 * gs::kRegBlocks, (P + 255) / 256); }

}  // namespace

extern "C" {

int gsplat_bilagrid_slice(const float *grid, int grid_w, int grid_h, int grid_l, const float *image, int rows, int cols,
                          float *out, void *stream) {
  if (int rc = check_grid(__func__, grid, grid_w, grid_h, grid_l)) return rc;
  GS_REQUIRE(rows > 0 && cols > 0, "image size must be positive");
  GS_REQUIRE(image != nullptr && out != nullptr, "image or out is null");
  GS_REQUIRE_DEV(grid); GS_REQUIRE_DEV(image); GS_REQUIRE_DEV(out);
  SliceArgs a = {};
  a.grid = {grid, grid_w, grid_h, grid_l};
  a.image = image; a.out = out; a.H = rows; a.W = cols;
  slice_kernel<false><<<pixel_blocks((long long)rows * cols), 256, 0, (hipStream_t)stream>>>(a);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

int gsplat_bilagrid_slice_backward(const float *grid, int grid_w, int grid_h, int grid_l, const float *image,
                                   const float *grad_out, int rows, int cols, int accumulate_grid, float *grad_image,
                                   float *grad_grid, void *stream) {
  if (int rc = check_grid(__func__, grid, grid_w, grid_h, grid_l)) return rc;
  GS_REQUIRE(rows > 0 && cols > 0, "image size must be positive");
  GS_REQUIRE(image != nullptr && grad_out != nullptr, "image or grad_out is null");
  GS_REQUIRE(grad_image != nullptr || grad_grid != nullptr, "grad_image and grad_grid are both null");
  const size_t image_bytes = (size_t)rows * cols * 3 * sizeof(float);
  GS_REQUIRE(!grad_image || (!overlap(grad_image, grad_out, image_bytes) && !overlap(grad_image, image, image_bytes)),
             "grad_image must not alias grad_out or image");
  const int ntx = (cols + kTile - 1) / kTile, nty = (rows + kTile - 1) / kTile;
  GS_REQUIRE((long long)ntx * nty < (1ll << 31), "image too large");
  GS_REQUIRE_DEV(grid); GS_REQUIRE_DEV(image); GS_REQUIRE_DEV(grad_out);
  if (grad_image) GS_REQUIRE_DEV(grad_image);
  if (grad_grid) GS_REQUIRE_DEV(grad_grid);
  hipStream_t st = (hipStream_t)stream;
  if (grad_image) {
    SliceArgs a = {};
    a.grid = {grid, grid_w, grid_h, grid_l};
    a.image = image; a.grad_out = grad_out; a.out = grad_image; a.H = rows; a.W = cols;
    slice_kernel<true><<<pixel_blocks((long long)rows * cols), 256, 0, st>>>(a);
    GS_LAUNCH_CHECK();
  }
  if (grad_grid) {
    SlabArgs a = {};
    a.grid = {grid, grid_w, grid_h, grid_l};
    a.image = image; a.grad_out = grad_out; a.H = rows; a.W = cols; a.ntx = ntx; a.nty = nty;
    a.add = accumulate_grid != 0; a.grad_grid = grad_grid;
    // the slots of a tile and the most tiles at one vertex, per axis, from the arithmetic the kernels use
    int most[2] = {0, 0};
    for (int axis = 0; axis < 2; ++axis) {
      const int n = axis ? grid_h : grid_w, size = axis ? rows : cols, nt = axis ? nty : ntx;
      int count[kMaxGridXY] = {}, widest = 1;
      for (int t = 0; t < nt; ++t) {
        int lo, hi;
        tile_vertex_range(t, size, n, lo, hi);
        widest = std::max(widest, hi - lo + 1);
        for (int v = lo; v <= hi; ++v) most[axis] = std::max(most[axis], ++count[v]);
      }
      (axis ? a.nj_s : a.ni_s) = widest;
    }
    const long long touching = (long long)most[0] * most[1];
    a.lanes = 1;
    while (a.lanes < 64 && touching > 8ll * a.lanes) a.lanes *= 2;
    const size_t slots = (size_t)a.ni_s * a.nj_s * grid_l * 12;
    gs::ScratchLock lock;
    gs::DeviceBuffer &slab = gs::scratch(gs::SCR_BILAGRID);
    if (int rc = slab.reserve((size_t)ntx * nty * slots * sizeof(double), st)) return rc;
    a.slab = slab.as<double>();
    grid_partial_kernel<<<(unsigned)(ntx * nty), 256, 0, st>>>(a);
    GS_LAUNCH_CHECK();
    const long long values = 12ll * grid_l * grid_h * grid_w;
    grid_finish_kernel<<<gs::div_up(values * a.lanes, 256), 256, 0, st>>>(a);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

int gsplat_bilagrid_tv_loss(const float *grid, int grid_w, int grid_h, int grid_l, float weight, int accumulate,
                            float *grad_grid, float *loss_out, void *stream) {
  if (int rc = check_grid(__func__, grid, grid_w, grid_h, grid_l)) return rc;
  GS_REQUIRE(grad_grid != nullptr || loss_out != nullptr, "grad_grid and loss_out are both null");
  GS_REQUIRE_DEV(grid);
  if (grad_grid) GS_REQUIRE_DEV(grad_grid);
  if (loss_out) GS_REQUIRE_DEV(loss_out);
  hipStream_t st = (hipStream_t)stream;
  if (grid_w == 1 && grid_h == 1 && grid_l == 1) {  // one colour affine: no pairs, the loss and its gradient are zero
    if (grad_grid && !accumulate) GS_HIP(hipMemsetAsync(grad_grid, 0, 12 * sizeof(float), st));
    if (loss_out) GS_HIP(hipMemsetAsync(loss_out, 0, sizeof(float), st));
    return GSPLAT_OK;
  }
  TvArgs a = {};
  a.grid = {grid, grid_w, grid_h, grid_l};
  const double lines = 12.0;
  a.cx = grid_w > 1 ? 1.0 / (lines * grid_l * grid_h * (grid_w - 1)) : 0.0;
  a.cy = grid_h > 1 ? 1.0 / (lines * grid_l * (grid_h - 1) * grid_w) : 0.0;
  a.cz = grid_l > 1 ? 1.0 / (lines * (grid_l - 1) * grid_h * grid_w) : 0.0;
  a.weight = (double)weight; a.add = accumulate != 0; a.grad = grad_grid;
  const int blocks = gs::reg_blocks(12ll * grid_l * grid_h * grid_w);
  gs::ScratchLock lock;
  if (loss_out) {
    gs::DeviceBuffer &acc = gs::scratch(gs::SCR_DEPTH_LOSS);
    if (int rc = acc.reserve(gs::kRegBlocks * sizeof(double))) return rc;
    a.partial = acc.as<double>();
  }
  tv_kernel<<<blocks, 256, 0, st>>>(a);
  GS_LAUNCH_CHECK();
  if (loss_out) {
    gs::reg_loss_finish_kernel<<<1, 64, 0, st>>>(a.partial, blocks, a.weight, loss_out);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

}  // extern "C"
