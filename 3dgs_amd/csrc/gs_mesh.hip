// gs_mesh.hip -- connected components of an indexed triangle mesh (gsplat_mesh_components) and the gather that drops
// components (gsplat_mesh_compact); definitions: include/gsplat_hip.h.  Off the training path: the cleanup behind
// ops.tsdf_extract (ops.mesh_components, ops.mesh_filter, Trainer.extract_mesh).
//
// Labelling is a lock-free union-find on the caller's `label` array used as the parent array: parent[v] <= v always, a
// root is parent[r] == r, hooking puts the LARGER root under the smaller, so a component's final root is its smallest
// vertex index.  The work per call is near-linear in the faces and does not grow with the mesh's diameter: paths are
// halved on the way up.  No grid-wide barrier, no waiting on another workgroup: a failed compare-and-swap means another
// thread made progress, and the loser goes on from the value the swap returned.
//
// What each kernel relies on, the eight XCDs' L2s not being coherent with each other:
//   check_faces_kernel  reads only the caller's faces (written before the launch) and ORs into one flag with an atomic.
//   init_kernel         plain stores of parent[v] = v and face_count[v] = 0; its readers run behind a kernel boundary.
//   hook_kernel         every read of parent is an agent-scope relaxed atomic load or the return of an atomicCAS / atomicMin,
//                       every write an atomicCAS (hooking a root) or an atomicMin (path halving): nothing is read plainly.
//   flatten_kernel      runs behind hook_kernel's boundary, so the forest is final; it still reads parent with atomic loads
//                       and writes label[v] with an atomic store, because it flattens in place and another thread may
//                       pass through v: either value it can see (v's old parent or v's root) leads to the same root.
//   count_kernel        runs behind flatten_kernel's boundary and reads label plainly; integer atomicAdd into face_count.
//   compact_kernel      a gather of arrays written before the launch; no atomics.
#include "gs_common.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int load_parent(const int *parent, int v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// v's root; on the way every visited vertex is pointed at its grandparent (atomicMin: a vertex's parent only ever moves to
// another of its ancestors, which all have smaller indices and lie on one path, so the minimum of two is an ancestor too)
__device__ __forceinline__ int find_root(int *parent, int v) {
  int p = load_parent(parent, v);
  while (p != v) {
    const int gp = load_parent(parent, p);
    if (gp != p) atomicMin(parent + v, gp);
    v = p;
    p = gp;
  }
  return v;
}

__device__ __forceinline__ void unite(int *parent, int a, int b) {
  int ra = find_root(parent, a), rb = find_root(parent, b);
  while (ra != rb) {
    const int hi = max(ra, rb), lo = min(ra, rb);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;           // hi was still a root: hooked
    ra = find_root(parent, old);     // somebody hooked hi first, under `old` < hi
    rb = find_root(parent, lo);
  }
}

__global__ __launch_bounds__(kBlock) void check_faces_kernel(const int *__restrict__ faces, int num_faces, int num_vertices,
                                                             int *__restrict__ flag) {
  const int f = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (f >= num_faces) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  const unsigned int n = (unsigned int)num_vertices;
  if ((unsigned int)a >= n || (unsigned int)b >= n || (unsigned int)c >= n) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void init_kernel(int num_vertices, int *__restrict__ parent, int *__restrict__ face_count) {
  const int v = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (v >= num_vertices) return;
  parent[v] = v;
  face_count[v] = 0;
}

// (the faces passed check_faces_kernel; the range test stays so that no out-of-range access can happen whatever they hold)
__device__ __forceinline__ bool load_face(const int *__restrict__ faces, int f, int num_vertices, int &a, int &b, int &c) {
  a = faces[3 * (size_t)f]; b = faces[3 * (size_t)f + 1]; c = faces[3 * (size_t)f + 2];
  const unsigned int n = (unsigned int)num_vertices;
  return (unsigned int)a < n && (unsigned int)b < n && (unsigned int)c < n;
}

__global__ __launch_bounds__(kBlock) void hook_kernel(const int *__restrict__ faces, int num_faces, int num_vertices,
                                                      int *parent) {
  const int f = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (f >= num_faces) return;
  int a, b, c;
  if (!load_face(faces, f, num_vertices, a, b, c)) return;
  unite(parent, a, b);
  unite(parent, a, c);
}

__global__ __launch_bounds__(kBlock) void flatten_kernel(int num_vertices, int *label) {
  const int v = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (v >= num_vertices) return;
  int r = v, p = load_parent(label, r);
  while (p != r) { r = p; p = load_parent(label, r); }
  __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One atomicAdd per wave and distinct label among its 64 faces (neighbouring faces mostly share one): the wave's lanes of
// the first pending lane's label are counted by a ballot and that lane adds their number.
__global__ __launch_bounds__(kBlock) void count_kernel(const int *__restrict__ faces, int num_faces, int num_vertices,
                                                       const int *__restrict__ label, int *__restrict__ face_count) {
  const int f = (int)(blockIdx.x * kBlock + threadIdx.x);
  int r = -1;
  if (f < num_faces) {
    int a, b, c;
    if (load_face(faces, f, num_vertices, a, b, c)) r = label[a];
  }
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const int rr = __shfl(r, lead);
    const unsigned long long same = __ballot(r == rr) & todo;
    if (lane == lead) atomicAdd(face_count + rr, __popcll(same));
    todo &= ~same;
  }
}

template <bool kColor>
__global__ __launch_bounds__(kBlock) void compact_kernel(const float *__restrict__ vertices, const float *__restrict__ colors,
                                                         const int *__restrict__ faces, int num_vertices, int num_faces,
                                                         const unsigned char *__restrict__ keep_vertex,
                                                         const long long *__restrict__ vertex_offset,
                                                         const long long *__restrict__ face_offset,
                                                         float *__restrict__ out_vertices, float *__restrict__ out_colors,
                                                         int *__restrict__ out_faces) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i < num_vertices && keep_vertex[i]) {
    const size_t o = (size_t)vertex_offset[i] * 3, s = (size_t)i * 3;
    out_vertices[o] = vertices[s]; out_vertices[o + 1] = vertices[s + 1]; out_vertices[o + 2] = vertices[s + 2];
    if constexpr (kColor) { out_colors[o] = colors[s]; out_colors[o + 1] = colors[s + 1]; out_colors[o + 2] = colors[s + 2]; }
  }
  if (i < num_faces) {
    int a, b, c;
    if (load_face(faces, i, num_vertices, a, b, c) && keep_vertex[a]) {
      const size_t o = (size_t)face_offset[i] * 3;
      out_faces[o] = (int)vertex_offset[a]; out_faces[o + 1] = (int)vertex_offset[b]; out_faces[o + 2] = (int)vertex_offset[c];
    }
  }
}

}  // namespace

extern "C" {

int gsplat_mesh_components(const int *faces, int num_faces, int num_vertices, int *label, int *face_count, int *rounds,
                           void *stream) {
  // (every check, the device's on the face indices included, before anything is written)
  GS_REQUIRE(num_faces >= 0 && num_vertices >= 0, "num_faces and num_vertices must not be negative");
  GS_REQUIRE(num_faces == 0 || num_vertices > 0, "faces without vertices");
  GS_REQUIRE(num_faces <= 0x7FFFFFFF / 3, "too many faces");
  if (num_vertices > 0) {
    GS_REQUIRE(label && face_count, "a required pointer is NULL");
    GS_REQUIRE_DEV(label); GS_REQUIRE_DEV(face_count);
  }
  if (num_faces > 0) {
    GS_REQUIRE(faces != nullptr, "faces is NULL");
    GS_REQUIRE_DEV(faces);
  }
  hipStream_t st = (hipStream_t)stream;
  if (rounds) *rounds = num_faces > 0 ? 1 : 0;
  if (num_vertices == 0) return GSPLAT_OK;
  const unsigned int vblocks = gs::div_up(num_vertices, kBlock), fblocks = gs::div_up(num_faces, kBlock);
  if (num_faces > 0) {
    gs::ScratchLock lock;  // library scratch and the pinned count words are process-wide
    int rc = gs::host_words().ensure();
    if (rc) return rc;
    gs::DeviceBuffer &misc = gs::scratch(gs::SCR_MISC);
    if ((rc = misc.reserve(64))) return rc;
    int *d_flag = misc.as<int>(), *h_flag = gs::host_words().p;
    GS_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    check_faces_kernel<<<fblocks, kBlock, 0, st>>>(faces, num_faces, num_vertices, d_flag);
    GS_LAUNCH_CHECK();
    GS_HIP(hipMemcpyAsync(h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));  // the call's one read-back
    GS_REQUIRE(h_flag[0] == 0, "a face index lies outside [0, num_vertices)");
  }
  init_kernel<<<vblocks, kBlock, 0, st>>>(num_vertices, label, face_count);
  GS_LAUNCH_CHECK();
  if (num_faces > 0) {
    hook_kernel<<<fblocks, kBlock, 0, st>>>(faces, num_faces, num_vertices, label);
    GS_LAUNCH_CHECK();
    flatten_kernel<<<vblocks, kBlock, 0, st>>>(num_vertices, label);
    GS_LAUNCH_CHECK();
    count_kernel<<<fblocks, kBlock, 0, st>>>(faces, num_faces, num_vertices, label, face_count);
    GS_LAUNCH_CHECK();
  }
  return GSPLAT_OK;
}

int gsplat_mesh_compact(const float *vertices, const float *colors, const int *faces, int num_vertices, int num_faces,
                        const unsigned char *keep_vertex, const long long *vertex_offset, const long long *face_offset,
                        float *out_vertices, float *out_colors, int *out_faces, void *stream) {
  GS_REQUIRE(num_faces >= 0 && num_vertices >= 0, "num_faces and num_vertices must not be negative");
  GS_REQUIRE(num_faces == 0 || num_vertices > 0, "faces without vertices");
  GS_REQUIRE(num_faces <= 0x7FFFFFFF / 3, "too many faces");
  GS_REQUIRE((colors != nullptr) == (out_colors != nullptr), "colors and out_colors go together");
  if (num_vertices == 0) return GSPLAT_OK;
  GS_REQUIRE(vertices && keep_vertex && vertex_offset && out_vertices, "a required pointer is NULL");
  GS_REQUIRE(num_faces == 0 || (faces && face_offset && out_faces), "a required pointer is NULL");
  GS_REQUIRE_DEV(vertices); GS_REQUIRE_DEV(keep_vertex); GS_REQUIRE_DEV(vertex_offset); GS_REQUIRE_DEV(out_vertices);
  if (colors) { GS_REQUIRE_DEV(colors); GS_REQUIRE_DEV(out_colors); }
  if (num_faces > 0) { GS_REQUIRE_DEV(faces); GS_REQUIRE_DEV(face_offset); GS_REQUIRE_DEV(out_faces); }
  hipStream_t st = (hipStream_t)stream;
  const unsigned int blocks = gs::div_up(num_vertices > num_faces ? num_vertices : num_faces, kBlock);
  if (colors)
    compact_kernel<true><<<blocks, kBlock, 0, st>>>(vertices, colors, faces, num_vertices, num_faces, keep_vertex,
                                                    vertex_offset, face_offset, out_vertices, out_colors, out_faces);
  else
    compact_kernel<false><<<blocks, kBlock, 0, st>>>(vertices, nullptr, faces, num_vertices, num_faces, keep_vertex,
                                                     vertex_offset, face_offset, out_vertices, nullptr, out_faces);
  GS_LAUNCH_CHECK();
  return GSPLAT_OK;
}

}  // extern "C"
