// Training targets from instance labels (the reference's preprocessing,
// hcat/train/train_utils.py, which runs as Python loops on the host):
//   hcu_label_keys        one 64-bit key per voxel of a colour / id label stack
//   hcu_pwl_scan          makePWL.find_closest (:62-93) for every voxel
//   hcu_label_moments     count and coordinate sums per id (CalculateCenterOfMass :218)
//   hcu_center_table      where each id sits in a centre volume (VectorToCenter :255)
//   hcu_vector_to_center  VectorToCenter (:240-274)
//   hcu_colormask_binary  colormask_to_mask (:175-187)
// Everything is integer work, or float64 values the host computed (the value
// table of the scan) or one IEEE division of two exact integers, so every
// result is bitwise the reference's.
//
// The scan: a workgroup owns 32 x 32 voxels of one z-slice and stages their
// keys with a 9-voxel halo in LDS (50 x 50 x 8 B = 20 KB; outside the stack
// reads 0, the reference's zero padding).  The (radius, angle) offsets come
// with the launch arguments and are read with wave-uniform indices (scalar
// loads); every lane walks the same sequence, four offsets per step (their
// loads in flight together: the scan is latency-bound), and keeps
// (closest, l0, l1) in registers.  A wave leaves the loop after a ring once a ballot shows every
// lane finished (both radii found, a labelled voxel, or outside the stack).
// The 32 x lanes of a row read consecutive 8-byte keys: no bank conflict.
#include "common.h"
#include "timing.h"
#include "hcunet.h"

namespace hcu {

constexpr int kPwlTile = 32;
constexpr int kPwlHalo = HCU_PWL_MAX_RADIUS;
constexpr int kPwlSpan = kPwlTile + 2 * kPwlHalo;   // 50

struct PwlTable {
  int ring_begin[HCU_PWL_MAX_RADIUS + 1];            // offsets of radius l: [ring_begin[l-1], ring_begin[l])
  int delta[HCU_PWL_MAX_OFFSETS];                     // dy * kPwlSpan + dx: a whole word, so a scalar load
  double value[HCU_PWL_MAX_RADIUS * HCU_PWL_MAX_RADIUS];   // [l0 - 1][l1 - 1]
};

template <typename T>
__device__ __forceinline__ uint64_t label_key(const T *p, int channels) {
  if (channels == 1) return (uint64_t)(uint32_t)p[0];
  return ((uint64_t)(uint32_t)p[0] << 32) | ((uint64_t)(uint32_t)p[1] << 16) | (uint64_t)(uint32_t)p[2];
}

template <typename T>
__global__ void __launch_bounds__(256)
label_keys_kernel(const T *labels, uint32_t nvox, int channels, int map_first, uint64_t *keys) {
  const uint64_t first = map_first ? label_key(labels, channels) : 0;   // (uniform: a scalar load)
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    const uint64_t k = label_key(labels + (size_t)i * channels, channels);
    keys[i] = k == first ? 0 : k;
  }
}

__global__ void __launch_bounds__(256)
pwl_scan_kernel(const uint64_t *keys, int Y, int X, const PwlTable tab, double *out) {
  __shared__ uint64_t tile[kPwlSpan * kPwlSpan];
  __shared__ double value[HCU_PWL_MAX_RADIUS * HCU_PWL_MAX_RADIUS];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kPwlTile, y0 = blockIdx.y * kPwlTile, z = blockIdx.z;
  const uint64_t *slice = keys + (size_t)z * Y * X;
  for (int i = tid; i < kPwlSpan * kPwlSpan; i += 256) {
    const int r = i / kPwlSpan, c = i - r * kPwlSpan;
    const int y = y0 - kPwlHalo + r, x = x0 - kPwlHalo + c;
    tile[i] = (y >= 0 && y < Y && x >= 0 && x < X) ? slice[(size_t)y * X + x] : 0;
  }
  if (tid < HCU_PWL_MAX_RADIUS * HCU_PWL_MAX_RADIUS) value[tid] = tab.value[tid];
  __syncthreads();
  const int lx = tid & 31;
  for (int ly = tid >> 5; ly < kPwlTile; ly += 8) {   // a wave: two rows of 32 voxels at a time
    const int y = y0 + ly, x = x0 + lx;
    const bool inside = y < Y && x < X;
    const int at = (ly + kPwlHalo) * kPwlSpan + lx + kPwlHalo;
    uint64_t closest = 0;
    int l0 = 0, l1 = 0;
    bool done = !inside || tile[at] != 0;
    for (int l = 1; l <= HCU_PWL_MAX_RADIUS; ++l) {
      if (__ballot(!done) == 0) break;
      const int kb = tab.ring_begin[l - 1], ke = tab.ring_begin[l];
      auto probe = [&](uint64_t p) {
        if (!done && p != 0) {
          if (closest == 0) {
            closest = p;
            l0 = l;
          } else if (p != closest) {
            l1 = l;
            done = true;
          }
        }
      };
      // four probes at a time: their scalar and LDS loads are in flight together
      int k = kb;
      for (; k + 4 <= ke; k += 4) {
        uint64_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = tile[at + tab.delta[k + j]];
#pragma unroll
        for (int j = 0; j < 4; ++j) probe(p[j]);
      }
      for (; k < ke; ++k) probe(tile[at + tab.delta[k]]);
    }
    if (inside)
      out[((size_t)z * Y + y) * X + x] = l1 ? value[(l0 - 1) * HCU_PWL_MAX_RADIUS + (l1 - 1)] : 0.0;
  }
}

constexpr int kMomentWindow = HCU_MOMENT_LDS_IDS;

__device__ __forceinline__ void add_u64(unsigned long long *p, unsigned long long v) { atomicAdd(p, v); }

__global__ void __launch_bounds__(256)
label_moments_kernel(const int *ids, uint32_t nvox, FastDiv fX, FastDiv fY, int n_ids,
                     unsigned long long *moments) {
  __shared__ unsigned long long acc[kMomentWindow * 4];
  for (int i = threadIdx.x; i < kMomentWindow * 4; i += 256) acc[i] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    const int id = ids[i];
    if (id < 0 || id >= n_ids) continue;   // not an id of the table: no address is formed from it
    int q, x, z, y;
    fX.divmod(i, q, x);
    fY.divmod((uint32_t)q, z, y);
    if (id < kMomentWindow) {   // LDS atomics
      unsigned long long *dst = acc + id * 4;
      add_u64(dst, 1ull);
      if (z) add_u64(dst + 1, (unsigned long long)z);
      if (y) add_u64(dst + 2, (unsigned long long)y);
      if (x) add_u64(dst + 3, (unsigned long long)x);
    } else {                    // outside the window: straight to global atomics
      unsigned long long *dst = moments + (size_t)id * 4;
      add_u64(dst, 1ull);
      if (z) add_u64(dst + 1, (unsigned long long)z);
      if (y) add_u64(dst + 2, (unsigned long long)y);
      if (x) add_u64(dst + 3, (unsigned long long)x);
    }
  }
  __syncthreads();
  const int nwin = n_ids < kMomentWindow ? n_ids : kMomentWindow;
  for (int i = threadIdx.x; i < nwin * 4; i += 256)
    if (acc[i]) add_u64(moments + i, acc[i]);
}

// The id a centre volume holds at a voxel, or 0: float64 values that are not
// whole numbers of [1, n_ids) match no id (np.where(center == id) of an integer id).
template <typename T>
__device__ __forceinline__ int centre_id(T v, int n_ids) {
  if constexpr (sizeof(T) == 8) {
    if (!(v >= 1.0 && v < (double)n_ids)) return 0;
    const int id = (int)v;
    return (double)id == v ? id : 0;
  } else {
    const long long w = (long long)v;
    return w >= 1 && w < n_ids ? (int)w : 0;
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
center_table_kernel(const T *center, uint32_t nvox, int n_ids, int *index, int *count) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    const int id = centre_id(center[i], n_ids);
    if (id) {
      atomicAdd(count + id, 1);
      atomicMax(index + id, (int)i);
    }
  }
}

__global__ void __launch_bounds__(256)
vector_to_center_kernel(const int *ids, uint32_t nvox, FastDiv fX, FastDiv fY, int Z, int Y, int X,
                        const int4 *centres, int n_ids, double *out) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    const int id = ids[i];
    double vz = 0.0, vy = 0.0, vx = 0.0;
    if (id > 0 && id < n_ids) {
      const int4 c = centres[id];
      if (c.w) {
        int q, x, z, y;
        fX.divmod(i, q, x);
        fY.divmod((uint32_t)q, z, y);
        vz = (double)(z - c.x) / (double)Z;
        vy = (double)(y - c.y) / (double)Y;
        vx = (double)(x - c.z) / (double)X;
      }
    }
    double *o = out + (size_t)i * 3;
    o[0] = vz;
    o[1] = vy;
    o[2] = vx;
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
colormask_binary_kernel(T *colormask, uint32_t nvox, uint8_t *mask) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    T *p = colormask + (size_t)i * 3;
    const bool any = p[0] != 0 || p[1] != 0 || p[2] != 0;
    if (any) {
      p[0] = 1;
      p[1] = 1;
      p[2] = 1;
    }
    mask[i] = any ? 255 : 0;   // (channel 0 * 255).astype(uint8), channel 0 now 0 or 1
  }
}

static int stack_voxels(const char *what, int Z, int Y, int X, uint32_t *nvox) {
  if (Z <= 0 || Y <= 0 || X <= 0) return fail(HCU_ERR_SHAPE, std::string(what) + ": empty stack");
  const int64_t n = (int64_t)Z * Y * X;
  if (n >= (1ll << 31)) return fail(HCU_ERR_UNSUPPORTED, std::string(what) + ": Z*Y*X must be below 2^31");
  *nvox = (uint32_t)n;
  return 0;
}
static int stream_grid(uint32_t nvox) { return (int)std::min<uint32_t>((nvox + 255u) / 256u, 2048u); }

}  // namespace hcu

using namespace hcu;

extern "C" int hcu_label_keys(const void *labels, int dtype, int Z, int Y, int X, int channels,
                              int map_first, uint64_t *keys, hcu_stream_t stream) {
  if (!labels || !keys) return fail(HCU_ERR_INVALID, "label_keys: null argument");
  uint32_t nvox;
  if (int rc = stack_voxels("label_keys", Z, Y, X, &nvox)) return rc;
  if (channels != 1 && channels != 3)
    return fail(HCU_ERR_SHAPE, "label_keys: a [Z,Y,X,3] colour stack or a [Z,Y,X] id stack");
  if (channels == 3 && dtype != HCU_U8 && dtype != HCU_U16)
    return fail(HCU_ERR_INVALID, "label_keys: a colour stack is uint8 or uint16");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(stream_grid(nvox));
  switch (dtype) {
    case HCU_U8:
      HCU_TIMED(s, "label_keys_kernel<u8>", 0.0, 0.0,
                HCU_LAUNCH(label_keys_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t *)labels, nvox,
                           channels, map_first, keys));
      break;
    case HCU_U16:
      HCU_TIMED(s, "label_keys_kernel<u16>", 0.0, 0.0,
                HCU_LAUNCH(label_keys_kernel<uint16_t>, grid, dim3(256), 0, s, (const uint16_t *)labels, nvox,
                           channels, map_first, keys));
      break;
    case HCU_I32:
    case HCU_U32:   // (ids are not negative: the same bits)
      HCU_TIMED(s, "label_keys_kernel<u32>", 0.0, 0.0,
                HCU_LAUNCH(label_keys_kernel<uint32_t>, grid, dim3(256), 0, s, (const uint32_t *)labels, nvox,
                           channels, map_first, keys));
      break;
    default:
      return fail(HCU_ERR_INVALID, "label_keys: labels are uint8, uint16, int32 or uint32");
  }
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_pwl_scan(const uint64_t *keys, int Z, int Y, int X, const int *offsets,
                            const int *ring_begin, const double *values, double *out,
                            hcu_stream_t stream) {
  if (!keys || !offsets || !ring_begin || !values || !out)
    return fail(HCU_ERR_INVALID, "pwl_scan: null argument");
  uint32_t nvox;
  if (int rc = stack_voxels("pwl_scan", Z, Y, X, &nvox)) return rc;
  if (Z > 65535 || cdiv(Y, kPwlTile) > 65535) return fail(HCU_ERR_UNSUPPORTED, "pwl_scan: more than 65535 slices or row tiles");
  PwlTable tab{};
  if (ring_begin[0] != 0) return fail(HCU_ERR_INVALID, "pwl_scan: ring_begin[0] must be 0");
  for (int l = 1; l <= HCU_PWL_MAX_RADIUS; ++l)
    if (ring_begin[l] < ring_begin[l - 1] || ring_begin[l] > HCU_PWL_MAX_OFFSETS)
      return fail(HCU_ERR_INVALID, "pwl_scan: ring_begin must ascend to at most HCU_PWL_MAX_OFFSETS");
  for (int l = 0; l <= HCU_PWL_MAX_RADIUS; ++l) tab.ring_begin[l] = ring_begin[l];
  for (int k = 0; k < ring_begin[HCU_PWL_MAX_RADIUS]; ++k) {
    const int dx = offsets[2 * k], dy = offsets[2 * k + 1];
    if (dx < -kPwlHalo || dx > kPwlHalo || dy < -kPwlHalo || dy > kPwlHalo)   // the LDS halo
      return fail(HCU_ERR_INVALID, "pwl_scan: an offset lies outside [-9, 9]");
    tab.delta[k] = dy * kPwlSpan + dx;
  }
  for (int i = 0; i < HCU_PWL_MAX_RADIUS * HCU_PWL_MAX_RADIUS; ++i) tab.value[i] = values[i];
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(X, kPwlTile), cdiv(Y, kPwlTile), Z);
  HCU_TIMED(s, "pwl_scan_kernel", 0.0, (double)nvox * 16.0,
            HCU_LAUNCH(pwl_scan_kernel, grid, dim3(256), 0, s, keys, Y, X, tab, out));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_label_moments(const int32_t *ids, int Z, int Y, int X, int n_ids, uint64_t *moments,
                                 hcu_stream_t stream) {
  if (!ids || !moments) return fail(HCU_ERR_INVALID, "label_moments: null argument");
  uint32_t nvox;
  if (int rc = stack_voxels("label_moments", Z, Y, X, &nvox)) return rc;
  if (n_ids <= 0) return fail(HCU_ERR_INVALID, "label_moments: n_ids must be positive");
  hipStream_t s = (hipStream_t)stream;
  HCU_HIP(hipMemsetAsync(moments, 0, (size_t)n_ids * 4 * sizeof(uint64_t), s));
  // few workgroups: each flushes its LDS window with one global atomic per touched word
  const dim3 grid(std::min(stream_grid(nvox), 512));
  HCU_TIMED(s, "label_moments_kernel", 0.0, (double)nvox * 4.0,
            HCU_LAUNCH(label_moments_kernel, grid, dim3(256), 0, s, ids, nvox, FastDiv((uint32_t)X),
                       FastDiv((uint32_t)Y), n_ids, (unsigned long long *)moments));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_center_table(const void *center, int dtype, int Z, int Y, int X, int n_ids,
                                int32_t *index, int32_t *count, hcu_stream_t stream) {
  if (!center || !index || !count) return fail(HCU_ERR_INVALID, "center_table: null argument");
  uint32_t nvox;
  if (int rc = stack_voxels("center_table", Z, Y, X, &nvox)) return rc;
  if (n_ids <= 0) return fail(HCU_ERR_INVALID, "center_table: n_ids must be positive");
  if (dtype != HCU_F64 && dtype != HCU_U8 && dtype != HCU_U16 && dtype != HCU_I32 && dtype != HCU_U32)
    return fail(HCU_ERR_INVALID, "center_table: the centre volume is float64, uint8, uint16, int32 or uint32");
  hipStream_t s = (hipStream_t)stream;
  HCU_HIP(hipMemsetAsync(index, 0xFF, (size_t)n_ids * sizeof(int32_t), s));   // -1: no voxel
  HCU_HIP(hipMemsetAsync(count, 0, (size_t)n_ids * sizeof(int32_t), s));
  const dim3 grid(stream_grid(nvox));
#define HCU_CENTER_CASE(T, tag)                                                                        \
  HCU_TIMED(s, "center_table_kernel<" tag ">", 0.0, 0.0,                                               \
            HCU_LAUNCH(center_table_kernel<T>, grid, dim3(256), 0, s, (const T *)center, nvox, n_ids, \
                       index, count))
  switch (dtype) {
    case HCU_F64: HCU_CENTER_CASE(double, "f64"); break;
    case HCU_U8: HCU_CENTER_CASE(uint8_t, "u8"); break;
    case HCU_U16: HCU_CENTER_CASE(uint16_t, "u16"); break;
    case HCU_I32: HCU_CENTER_CASE(int32_t, "i32"); break;
    default: HCU_CENTER_CASE(uint32_t, "u32"); break;
  }
#undef HCU_CENTER_CASE
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_vector_to_center(const int32_t *ids, int Z, int Y, int X, const int32_t *centres,
                                    int n_ids, double *out, hcu_stream_t stream) {
  if (!ids || !centres || !out) return fail(HCU_ERR_INVALID, "vector_to_center: null argument");
  uint32_t nvox;
  if (int rc = stack_voxels("vector_to_center", Z, Y, X, &nvox)) return rc;
  if (n_ids <= 0) return fail(HCU_ERR_INVALID, "vector_to_center: n_ids must be positive");
  if ((uintptr_t)centres % 16) return fail(HCU_ERR_INVALID, "vector_to_center: centres must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  HCU_TIMED(s, "vector_to_center_kernel", 0.0, (double)nvox * 28.0,
            HCU_LAUNCH(vector_to_center_kernel, dim3(stream_grid(nvox)), dim3(256), 0, s, ids, nvox,
                       FastDiv((uint32_t)X), FastDiv((uint32_t)Y), Z, Y, X, (const int4 *)centres, n_ids, out));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_colormask_binary(void *colormask, int dtype, int Z, int Y, int X, uint8_t *mask,
                                    hcu_stream_t stream) {
  if (!colormask || !mask) return fail(HCU_ERR_INVALID, "colormask_binary: null argument");
  uint32_t nvox;
  if (int rc = stack_voxels("colormask_binary", Z, Y, X, &nvox)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(stream_grid(nvox));
  switch (dtype) {
    case HCU_U8:
      HCU_TIMED(s, "colormask_binary_kernel<u8>", 0.0, 0.0,
                HCU_LAUNCH(colormask_binary_kernel<uint8_t>, grid, dim3(256), 0, s, (uint8_t *)colormask, nvox,
                           mask));
      break;
    case HCU_U16:
      HCU_TIMED(s, "colormask_binary_kernel<u16>", 0.0, 0.0,
                HCU_LAUNCH(colormask_binary_kernel<uint16_t>, grid, dim3(256), 0, s, (uint16_t *)colormask,
                           nvox, mask));
      break;
    case HCU_I32:
    case HCU_U32:
      HCU_TIMED(s, "colormask_binary_kernel<u32>", 0.0, 0.0,
                HCU_LAUNCH(colormask_binary_kernel<uint32_t>, grid, dim3(256), 0, s, (uint32_t *)colormask,
                           nvox, mask));
      break;
    default:
      return fail(HCU_ERR_INVALID, "colormask_binary: the colour mask is uint8, uint16, int32 or uint32");
  }
  HCU_CHECK_LAUNCH();
  return 0;
}
