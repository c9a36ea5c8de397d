// Cell objects from a label volume (the reference's generate_cell_objects,
// hcat/segment.py:508-560, and HairCell, hcat/haircell.py:5-85, which loop over
// the ids on the host with a full-volume mask per id):
//   hcu_cell_boxes   inclusive bounding box of every id, one pass
//   hcu_cell_stats   per cell and channel: voxel count, count per z plane,
//                    minimum of the clipped box, mean, standard deviation and
//                    the two middle order statistics of the cell's values
//
// The boxes: integer min / max atomics, the first HCU_BOX_LDS_IDS ids in an
// LDS table a workgroup flushes with one global atomic per touched word, the
// rest straight to global.  A lane reads the word first and skips the atomic
// when its coordinate would not move it (the word only ever moves one way, so
// a stale read costs an atomic, never a result): the background's voxels, most
// of the volume, settle their box after a few waves.
//
// The statistics: one workgroup per (cell, channel) walks the clipped box
// x0:x1, y0:y1, z0:z1 (the maximum faces dropped, as the reference slices) by
// flat index, so the 256 lanes stay busy whatever the box's shape; labels and
// image of a box stay in L2 between the walks.
//   walk 1  count per plane (LDS integer atomics), minimum over all channels
//           (an LDS atomicMin on the order-preserving key), the float64 sums
//           of the raw and of the mapped values of the cell's voxels
//   walk 2  float64 sum of (g - mean)^2
//   walks 3..6  exact radix select of the ranks floor((n-1)/2) and floor(n/2)
//           on the float32 bit pattern, 8 bits a pass, most significant first:
//           an LDS histogram per rank of the keys that share the rank's
//           prefix (one histogram while the two prefixes agree); a wave per
//           rank finds its bucket with a shuffle scan
// A walk is bound by load latency (the box sits in L2, a workgroup has the CU
// nearly to itself), so a lane issues the loads of kWalkBatch voxels before it
// uses any.
// Float sums go lane -> wave (shuffles) -> workgroup (LDS) in a fixed order:
// two calls give the same bits.  No float atomics, no compaction, no sort.
#include "common.h"
#include "timing.h"
#include "hcunet.h"

#include <cmath>

namespace hcu {

constexpr int kBoxWindow = HCU_BOX_LDS_IDS;
constexpr int kMaxPlanes = HCU_CELL_MAX_PLANES;

__device__ __forceinline__ int peek(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// boxes words: the minima as unsigned (empty: 0xFFFFFFFF), the maxima as signed (empty: -1)
__device__ __forceinline__ void box_update(int *dst, int x, int y, int z) {
  if ((unsigned)x < (unsigned)peek(dst + 0)) atomicMin((unsigned *)dst + 0, (unsigned)x);
  if ((unsigned)y < (unsigned)peek(dst + 1)) atomicMin((unsigned *)dst + 1, (unsigned)y);
  if ((unsigned)z < (unsigned)peek(dst + 2)) atomicMin((unsigned *)dst + 2, (unsigned)z);
  if (x > peek(dst + 3)) atomicMax(dst + 3, x);
  if (y > peek(dst + 4)) atomicMax(dst + 4, y);
  if (z > peek(dst + 5)) atomicMax(dst + 5, z);
}

__global__ void __launch_bounds__(256)
cell_boxes_kernel(const int *ids, uint32_t nvox, FastDiv fZ, FastDiv fY, int n_ids, int *boxes) {
  __shared__ int tab[kBoxWindow * 6];
  for (int i = threadIdx.x; i < kBoxWindow * 6; i += 256) tab[i] = -1;
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    const int id = ids[i];
    if (id < 0 || id >= n_ids) continue;   // not an id of the table: no address is formed from it
    int q, x, y, z;
    fZ.divmod(i, q, z);
    fY.divmod((uint32_t)q, x, y);
    if (id < kBoxWindow) box_update(tab + id * 6, x, y, z);
    else box_update(boxes + (size_t)id * 6, x, y, z);
  }
  __syncthreads();
  const int nwin = n_ids < kBoxWindow ? n_ids : kBoxWindow;
  for (int i = threadIdx.x; i < nwin * 6; i += 256) {
    const int v = tab[i];
    if (v == -1) continue;
    if (i % 6 < 3) atomicMin((unsigned *)boxes + i, (unsigned)v);
    else atomicMax(boxes + i, v);
  }
}

// float32 bits <-> a key whose unsigned order is the numeric order (-0 below +0)
__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <int DT>
__device__ __forceinline__ float img_at(const void *img, size_t i) {
  if constexpr (DT == HCU_F32) return static_cast<const float *>(img)[i];
  else if constexpr (DT == HCU_F16) return (float)static_cast<const _Float16 *>(img)[i];
  else return bf2f(static_cast<const uint16_t *>(img)[i]);
}

__device__ __forceinline__ FastDiv device_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  f.s = s;
  f.m = (uint32_t)((((1ull << s) - d) << 32) / d + 1);
  return f;
}

// The workgroup's sum of v, the same bits in every thread and every call:
// within a wave by halving shuffles, then the four waves in order.
__device__ __forceinline__ double block_sum(double v, double *slot) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();   // slot free again
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

struct CellBox {
  int x0, y0, z0, bz;
  uint32_t n;          // voxels of the clipped box
  FastDiv fz, fy;
  int Y, Z;
  // flat index of the clipped box -> linear index of the volume and the z plane inside the box
  __device__ __forceinline__ uint32_t at(uint32_t i, int &z) const {
    int q, x, y;
    fz.divmod(i, q, z);
    fy.divmod((uint32_t)q, x, y);
    return ((uint32_t)(x0 + x) * (uint32_t)Y + (uint32_t)(y0 + y)) * (uint32_t)Z + (uint32_t)(z0 + z);
  }
};

constexpr int kWalkBatch = 4;   // voxels a lane has in flight: a walk is bound by load latency, not by bytes

// f(g, z) for every voxel of the clipped box that carries `id` (id > 0), g its value in `chan`; a
// lane's voxels in ascending flat index.  A batch's loads are issued before any is used; the slots
// past the box re-read the lane's first voxel and are dropped.
template <int DT, typename F>
__device__ __forceinline__ void for_cell_values(const CellBox &b, const int *labels, const void *chan, int id,
                                                F &&f) {
  for (uint32_t i0 = threadIdx.x; i0 < b.n; i0 += 256u * kWalkBatch) {
    int lab[kWalkBatch], z[kWalkBatch];
    float g[kWalkBatch];
#pragma unroll
    for (int u = 0; u < kWalkBatch; ++u) {
      const uint32_t i = i0 + 256u * u;
      const bool in = i < b.n;
      const uint32_t v = b.at(in ? i : i0, z[u]);
      lab[u] = labels[v];
      g[u] = img_at<DT>(chan, v);
      if (!in) lab[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < kWalkBatch; ++u)
      if (lab[u] == id) f(g[u], z[u]);
  }
}

// The bucket of hist[256] that holds rank `rank` (0-based, below the histogram's total) and the rank
// inside it.  One whole wave: lane l owns buckets 4l..4l+3, an inclusive scan over the lanes.
__device__ __forceinline__ void select_bucket(const int *h, int rank, int *bucket, int *left) {
  const int l = threadIdx.x & 63;
  const int a0 = h[4 * l], a1 = h[4 * l + 1], a2 = h[4 * l + 2], a3 = h[4 * l + 3];
  const int own = a0 + a1 + a2 + a3;
  int incl = own;
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (l >= off) incl += t;
  }
  const int excl = incl - own;
  if (rank >= excl && rank < incl) {   // one lane
    int r = rank - excl, bkt = 4 * l;
    if (r >= a0) {
      r -= a0, ++bkt;
      if (r >= a1) {
        r -= a1, ++bkt;
        if (r >= a2) r -= a2, ++bkt;
      }
    }
    *bucket = bkt;
    *left = r;
  }
}

template <int DT>
__global__ void __launch_bounds__(256)
cell_stats_kernel(const int *labels, const int *boxes, const void *img, int64_t cstride, int C, int X, int Y,
                  int Z, int *count, int *plane_count, float *box_min, double *mean, double *stdev,
                  float *median) {
  __shared__ int plane[kMaxPlanes];
  __shared__ int hist[2][256];
  __shared__ double slot[4];
  __shared__ int s_count, s_flags;
  __shared__ uint32_t s_minkey;
  __shared__ int s_bucket[2], s_rank[2];
  const int tid = threadIdx.x;
  const int id = blockIdx.x / C, c = blockIdx.x - id * C;   // (uniform)
  const int *bx = boxes + (size_t)id * 6;
  // the box as the caller's table gives it, held inside the volume: no address outside is formed
  const int x0 = max(bx[0], 0), y0 = max(bx[1], 0), z0 = max(bx[2], 0);
  const int x1 = min(bx[3], X - 1), y1 = min(bx[4], Y - 1), z1 = min(bx[5], Z - 1);
  const int ex = id == 0 ? 0 : max(x1 - x0, 0), ey = max(y1 - y0, 0), ez = max(z1 - z0, 0);
  CellBox b;
  b.x0 = x0, b.y0 = y0, b.z0 = z0, b.bz = ez, b.Y = Y, b.Z = Z;
  b.n = (uint32_t)ex * (uint32_t)ey * (uint32_t)ez;
  b.fz = device_fastdiv((uint32_t)max(ez, 1));
  b.fy = device_fastdiv((uint32_t)max(ey, 1));
  const void *chan = static_cast<const char *>(img) + (size_t)c * (size_t)cstride * (DT == HCU_F32 ? 4 : 2);

  for (int z = tid; z < ez; z += 256) plane[z] = 0;
  if (tid == 0) {
    s_count = 0;
    s_flags = 0;
    s_minkey = f2key(INFINITY);
  }
  __syncthreads();

  // walk 1
  double sum_raw = 0.0, sum_map = 0.0;
  float mn = INFINITY;
  int flags = 0;   // 1: a NaN in the clipped box (any channel), 2: a NaN among the cell's values
  for (uint32_t i0 = tid; i0 < b.n; i0 += 256u * kWalkBatch) {
    uint32_t v[kWalkBatch];
    int lab[kWalkBatch], z[kWalkBatch];
    float g[kWalkBatch];
#pragma unroll
    for (int u = 0; u < kWalkBatch; ++u) {   // (a slot past the box re-reads the lane's first voxel: the minimum does not mind)
      const uint32_t i = i0 + 256u * u;
      const bool in = i < b.n;
      v[u] = b.at(in ? i : i0, z[u]);
      lab[u] = labels[v[u]];
      if (!in) lab[u] = -1;
      g[u] = 0.0f;
    }
    for (int cc = 0; cc < C; ++cc) {
      float f[kWalkBatch];
#pragma unroll
      for (int u = 0; u < kWalkBatch; ++u) f[u] = img_at<DT>(img, (size_t)cc * (size_t)cstride + v[u]);
#pragma unroll
      for (int u = 0; u < kWalkBatch; ++u) {
        if (f[u] != f[u]) flags |= 1;
        else mn = f[u] < mn ? f[u] : mn;
        if (cc == c) g[u] = f[u];
      }
    }
#pragma unroll
    for (int u = 0; u < kWalkBatch; ++u)
      if (lab[u] == id) {
        atomicAdd(&plane[z[u]], 1);
        if (g[u] != g[u]) flags |= 2;
        sum_raw += (double)g[u];
        sum_map += (double)(g[u] * 0.5f + 0.5f);
      }
  }
  atomicMin(&s_minkey, f2key(mn));
  if (flags) atomicOr(&s_flags, flags);
  __syncthreads();
  for (int z = tid; z < ez; z += 256)
    if (plane[z]) atomicAdd(&s_count, plane[z]);
  sum_raw = block_sum(sum_raw, slot);   // (its barriers publish s_count too)
  sum_map = block_sum(sum_map, slot);
  const int n = s_count;
  flags = s_flags;
  const float bmin = (flags & 1) ? __uint_as_float(0x7fc00000u) : key2f(s_minkey);
  const bool map = bmin < 0.0f;   // false for a NaN: the reference's image.min() < 0
  if (c == 0) {
    for (int z = tid; z < Z; z += 256)
      plane_count[(size_t)id * Z + z] = (z >= z0 && z < z0 + ez) ? plane[z - z0] : 0;
    if (tid == 0) {
      count[id] = n;
      box_min[id] = bmin;
    }
  }
  const size_t o = (size_t)id * C + c;
  if (n <= 1 || (flags & 2)) {
    if (tid == 0) {
      const double qnan = __longlong_as_double(0x7ff8000000000000ll);
      mean[o] = qnan;
      stdev[o] = qnan;
      median[2 * o] = __uint_as_float(0x7fc00000u);
      median[2 * o + 1] = __uint_as_float(0x7fc00000u);
    }
    return;
  }
  const double mu = (map ? sum_map : sum_raw) / (double)n;

  // walk 2
  double ss = 0.0;
  for_cell_values<DT>(b, labels, chan, id, [&](float g, int) {
    if (map) g = g * 0.5f + 0.5f;
    const double d = (double)g - mu;
    ss += d * d;
  });
  ss = block_sum(ss, slot);

  // walks 3..6: the ranks r[0] <= r[1] among the keys that carry prefix[j] in the bits above `shift`
  uint32_t prefix[2] = {0u, 0u}, himask = 0u;
  int r[2] = {(n - 1) / 2, n / 2};
  for (int shift = 24; shift >= 0; shift -= 8) {
    const bool same = prefix[0] == prefix[1];
    hist[0][tid] = 0;
    hist[1][tid] = 0;
    __syncthreads();
    for_cell_values<DT>(b, labels, chan, id, [&](float g, int) {
      if (map) g = g * 0.5f + 0.5f;
      const uint32_t k = f2key(g);
      const int bucket = (int)((k >> shift) & 255u);
      if ((k & himask) == prefix[0]) atomicAdd(&hist[0][bucket], 1);
      if (!same && (k & himask) == prefix[1]) atomicAdd(&hist[1][bucket], 1);
    });
    __syncthreads();
    if (tid < 128) {   // two waves: a rank each
      const int j = tid >> 6;
      select_bucket(hist[same ? 0 : j], r[j], &s_bucket[j], &s_rank[j]);
    }
    __syncthreads();
    for (int j = 0; j < 2; ++j) {
      prefix[j] |= (uint32_t)s_bucket[j] << shift;
      r[j] = s_rank[j];
    }
    himask |= 255u << shift;
    __syncthreads();   // s_bucket / hist free again
  }
  if (tid == 0) {
    mean[o] = mu;
    stdev[o] = sqrt(ss / (double)n);
    median[2 * o] = key2f(prefix[0]);
    median[2 * o + 1] = key2f(prefix[1]);
  }
}

static int volume_voxels(const char *what, int X, int Y, int Z, uint32_t *nvox) {
  if (X <= 0 || Y <= 0 || Z <= 0) return fail(HCU_ERR_SHAPE, std::string(what) + ": empty volume");
  const int64_t n = (int64_t)X * Y * Z;
  if (n >= (1ll << 31)) return fail(HCU_ERR_UNSUPPORTED, std::string(what) + ": X*Y*Z must be below 2^31");
  *nvox = (uint32_t)n;
  return 0;
}

}  // namespace hcu

using namespace hcu;

extern "C" int hcu_cell_boxes(const int32_t *ids, int X, int Y, int Z, int n_ids, int32_t *boxes,
                              hcu_stream_t stream) {
  if (!ids || !boxes) return fail(HCU_ERR_INVALID, "cell_boxes: null argument");
  uint32_t nvox;
  if (int rc = volume_voxels("cell_boxes", X, Y, Z, &nvox)) return rc;
  if (n_ids <= 0) return fail(HCU_ERR_INVALID, "cell_boxes: n_ids must be positive");
  hipStream_t s = (hipStream_t)stream;
  HCU_HIP(hipMemsetAsync(boxes, 0xFF, (size_t)n_ids * 6 * sizeof(int32_t), s));   // no voxel: -1
  // few workgroups: each flushes its LDS window with one global atomic per touched word
  const dim3 grid((int)std::min<uint32_t>((nvox + 255u) / 256u, 512u));
  HCU_TIMED(s, "cell_boxes_kernel", 0.0, (double)nvox * 4.0,
            HCU_LAUNCH(cell_boxes_kernel, grid, dim3(256), 0, s, ids, nvox, FastDiv((uint32_t)Z),
                       FastDiv((uint32_t)Y), n_ids, boxes));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_cell_stats(const int32_t *ids, const int32_t *boxes, const void *image, int dtype,
                              int64_t chan_stride, int C, int X, int Y, int Z, int n_ids, int32_t *count,
                              int32_t *plane_count, float *box_min, double *mean, double *std, float *median,
                              hcu_stream_t stream) {
  if (!ids || !boxes || !image || !count || !plane_count || !box_min || !mean || !std || !median)
    return fail(HCU_ERR_INVALID, "cell_stats: null argument");
  uint32_t nvox;
  if (int rc = volume_voxels("cell_stats", X, Y, Z, &nvox)) return rc;
  if (n_ids <= 0 || C <= 0) return fail(HCU_ERR_INVALID, "cell_stats: n_ids and C must be positive");
  if (chan_stride < (int64_t)nvox) return fail(HCU_ERR_INVALID, "cell_stats: chan_stride below X*Y*Z");
  if (Z > kMaxPlanes) return fail(HCU_ERR_UNSUPPORTED, "cell_stats: more than HCU_CELL_MAX_PLANES z planes");
  if ((int64_t)n_ids * C >= (1ll << 31)) return fail(HCU_ERR_UNSUPPORTED, "cell_stats: n_ids * C must be below 2^31");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(n_ids * C));
#define HCU_CELL_CASE(DT, tag)                                                                             \
  HCU_TIMED(s, "cell_stats_kernel<" tag ">", 0.0, 0.0,                                                    \
            HCU_LAUNCH(cell_stats_kernel<DT>, grid, dim3(256), 0, s, ids, boxes, image, chan_stride, C, X, \
                       Y, Z, count, plane_count, box_min, mean, std, median))
  switch (dtype) {
    case HCU_F32: HCU_CELL_CASE(HCU_F32, "f32"); break;
    case HCU_F16: HCU_CELL_CASE(HCU_F16, "f16"); break;
    case HCU_BF16: HCU_CELL_CASE(HCU_BF16, "bf16"); break;
    default: return fail(HCU_ERR_INVALID, "cell_stats: the image is fp32, fp16 or bf16");
  }
#undef HCU_CELL_CASE
  HCU_CHECK_LAUNCH();
  return 0;
}
