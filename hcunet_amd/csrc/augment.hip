// Input path with random crops and intensity augmentation (hcu_ingest_jobs):
// the reference's training recipe (tests/transforms_test.py:22-39) on the
// device, one launch for every volume of a batch.  A job reads a window of a
// raw [Z][Y][X][C] uint16 / uint8 stack through an origin or an index map per
// axis (random_crop hcat/transforms.py:337-396, nul_crop :460-489), selects
// channels (remove_channel :590-613), runs the recorded per-voxel program in
// float64 in recorded order (normalize :257-283, random_intensity :301-334,
// drop_channel :285-298, clean_image :616-631, random_gamma :186-197, spekle
// :159-183) and rounds as torch does (float64 -> float32 -> fp16), writing
// [C'][ox][oy][oz] fp16.
//
// random_rotate (:230-254) is an addressing mode of the load phase, not a pass
// of its own: with J.rot the window / maps describe the pre-rotation view and
// every output (x, y) gathers its nearest source voxel of that view, exactly as
// scipy.ndimage.rotate(order=0, mode='constant', reshape=False) picks it --
// float64 coordinates with every product and sum rounded on its own (fused
// multiply-adds move the .5 ties), computed once per tile column and reused
// for its z rows.  A voxel whose source lies outside issues no load, starts
// from 0.0 at step J.fill_after and runs the steps that were recorded after
// the rotation.  Neighbouring output rows reuse the same source cache lines,
// so the gather goes through L2 / the vector cache, not through LDS.
//
// A workgroup owns a tile of 32 x by ty y by tz z output voxels of one job
// (all its channels), staged in LDS: the reads run along (x, c), the source's
// contiguous direction, and the writes along (y, z), the destination's -- a
// tile that spans the whole z extent writes runs of ty * oz halves.  The job
// and its tiling are found per workgroup from the table (block-uniform).
// Every output element is written.
#include "common.h"
#include "timing.h"
#include "hcunet.h"
#include <cmath>
#include <cstring>

namespace hcu {

constexpr int kAugTX = 32;
constexpr int kAugTileHalves = 16384;                                     // 32 KB of outputs per tile
constexpr int kAugLds = kAugTileHalves + HCU_INGEST_MAX_C * kAugTX * 3;   // + row padding

struct AugTiling {
  int tz, ty, pitch, ntx, nty, ntz, tiles;
};
// tz = the whole z extent up to 32; ty as many rows (<= 8) as the LDS tile
// holds; pitch = halves per (c, x) row of the LDS tile, 2 mod 4 so that the 32
// x lanes of the load phase land on 32 different banks.
__host__ __device__ inline AugTiling aug_tiling(int n_chan, int ox, int oy, int oz) {
  AugTiling t;
  t.tz = oz < 32 ? oz : 32;
  int ty = kAugTileHalves / (n_chan * kAugTX * t.tz);
  ty = ty > 8 ? 8 : ty;
  t.ty = ty > oy ? oy : ty;
  const int run = t.ty * t.tz;
  t.pitch = run + (6 - run % 4) % 4;
  t.ntx = (ox + kAugTX - 1) / kAugTX;
  t.nty = (oy + t.ty - 1) / t.ty;
  t.ntz = (oz + t.tz - 1) / t.tz;
  t.tiles = t.ntx * t.nty * t.ntz;
  return t;
}

// Philox-4x32-10 (Salmon et al., SC'11): counter c, key k -> 4 random words.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// Two standard normals per (key, job, step, output voxel, channel pair):
// Box-Muller on two 53-bit uniforms of (0, 1), float64; the even channel of
// the pair takes the cosine branch, the odd one the sine branch.
__device__ __forceinline__ void aug_normal2(uint32_t key, uint32_t job, uint32_t step, uint32_t voxel,
                                            uint32_t pair, double &n0, double &n1) {
  uint32_t c[4] = {voxel, pair, job, step};
  philox4x32_10(c, key, 0x68637561u);
  const double u1 = ((double)((((uint64_t)c[0] << 32) | c[1]) >> 11) + 0.5) * 0x1p-53;
  const double u2 = ((double)((((uint64_t)c[2] << 32) | c[3]) >> 11) + 0.5) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  n0 = r * cs;
  n1 = r * sn;
}

// The steps without noise, on one value with its channel's operands.
__device__ __forceinline__ double aug_pointwise(int kind, double v, double a, double b) {
  switch (kind) {
    case HCU_AUG_NORMALIZE:
      return (v + -a) / b;
    case HCU_AUG_INTENSITY:
      v -= a;
      if (v < 0) v = 0;
      if (isnan(v)) v = 0;
      return isinf(v) ? 1.0 : v;
    case HCU_AUG_DROP:
      return a != 0 ? 0.0 : v;
    case HCU_AUG_CLEAN:
      if (isnan(v)) v = 0;
      return isinf(v) ? 1.0 : v;
    case HCU_AUG_GAMMA:
      return pow(v, a);
    default:
      return v;
  }
}
__device__ __forceinline__ double aug_add_noise(double v, double gamma, double n) {
  v = v + (double)(float)(gamma * n);   // np.float32(noise)
  if (v < 0) v = 0;
  return v > 1 ? 1.0 : v;
}

// Source element k of a voxel whose C * es <= 16 bytes were loaded into w.
template <int ES>
__device__ __forceinline__ uint32_t aug_elem(const uint32_t (&w)[4], int k) {
  const int bo = k * ES;
  const uint32_t d = bo < 8 ? (bo < 4 ? w[0] : w[1]) : (bo < 12 ? w[2] : w[3]);
  return (d >> ((bo & 3) * 8)) & (ES == 2 ? 0xffffu : 0xffu);
}

// Source voxel (sx, sy) of the pre-rotation view for voxel (u, v) of the
// rotated view; false: outside (the constant).  Contraction is switched off
// for this code: the device compiler would otherwise fuse u * c + v * s into
// an FMA, whose single rounding differs from scipy's at exact .5 ties.  (The
// operators are written out: the __dmul_rn / __dadd_rn of the device headers
// are plain * and + that inline with their own contraction flags.)  The inside
// test is written with positive comparisons, so a NaN coordinate is outside,
// and the conversion to int comes after it (0 <= floor(c + .5) <= n - 1 then).
__device__ __forceinline__ bool aug_rot_source(const hcu_ingest_job &J, int u, int v, int &sx, int &sy) {
#pragma clang fp contract(off)
  const double du = (double)u, dv = (double)v;
  const double xa = du * J.rot_m[0], xb = dv * J.rot_m[1];
  const double ya = du * J.rot_m[2], yb = dv * J.rot_m[3];
  const double xs = xa + xb, ys = ya + yb;
  const double cx = xs + J.rot_off[0], cy = ys + J.rot_off[1];
  const bool inside = cx >= 0.0 && cx <= (double)(J.rot_nx - 1) && cy >= 0.0 && cy <= (double)(J.rot_ny - 1);
  if (!inside) return false;
  sx = (int)floor(cx + 0.5);
  sy = (int)floor(cy + 0.5);
  return true;
}

template <typename T, bool ROT>
__device__ __forceinline__ void aug_job_tile(const hcu_ingest_job &J, const AugTiling &jt, int job, int t,
                                             uint16_t *tile) {
  constexpr int ES = (int)sizeof(T);
  const int tid = threadIdx.x;
  const int nc = J.n_chan, C = J.C, Y = J.Y, X = J.X;
  const int ox = J.ox, oy = J.oy, oz = J.oz;
  const int ty = jt.ty, tz = jt.tz, pitch = jt.pitch;
  const int xb = (t % jt.ntx) * kAugTX, yb = (t / jt.ntx % jt.nty) * ty, zb = (t / (jt.ntx * jt.nty)) * tz;
  const int nx = min(kAugTX, ox - xb), ny = min(ty, oy - yb), nz = min(tz, oz - zb);
  const T *src = (const T *)J.src;
  const int *xmap = J.xmap_dev, *ymap = J.ymap_dev;
  const int vb = C * ES;   // bytes of one voxel: loaded as one vector when a power of two <= 16
  const bool vec = (vb == 1 || vb == 2 || vb == 4 || vb == 8 || vb == 16) && ((uintptr_t)J.src % vb) == 0;
  const double scale = J.scale;
  const int nsteps = J.n_steps;

  // load: x fastest (the source's contiguous direction), program, LDS [c][x][y][z]
  const int nvox = kAugTX * ty * tz;
  // ROT: the source of this thread's tile column.  xi never changes between a
  // thread's iterations and yi only when ty does not divide 8, so the
  // coordinates are computed once per (x, y) and reused for the z rows.
  int col_y = -1, rx = 0, ry = 0;
  bool inside = true;
  for (int i = tid; i < nvox; i += 256) {
    const int xi = i & (kAugTX - 1), r = i >> 5, yi = r % ty, zi = r / ty;
    if (xi >= nx || yi >= ny || zi >= nz) continue;
    int vx = xb + xi, vy = yb + yi;   // voxel of the (pre-rotation) view
    if constexpr (ROT) {
      if (yi != col_y) {
        inside = aug_rot_source(J, J.rot_px + vx, J.rot_py + vy, rx, ry);
        col_y = yi;
      }
      vx = inside ? rx : 0;
      vy = inside ? ry : 0;
    }
    const int sx = xmap ? xmap[vx] : J.x0 + vx;
    const int sy = ymap ? ymap[vy] : J.y0 + vy;
    const int sz = J.z0 + zb + zi;
    const uint32_t voff = ((uint32_t)sz * Y + sy) * X + sx;                 // < 2^31 / (C * ES): validated
    const uint32_t ovox = ((uint32_t)(xb + xi) * oy + yb + yi) * oz + zb + zi;
    uint32_t w[4] = {0, 0, 0, 0};
    if (vec && (!ROT || inside)) {
      const char *p = (const char *)src + (size_t)voff * vb;
      if (vb == 16) {
        const uint4 q = *(const uint4 *)p;
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
      } else if (vb == 8) {
        const uint2 q = *(const uint2 *)p;
        w[0] = q.x; w[1] = q.y;
      } else if (vb == 4) {
        w[0] = *(const uint32_t *)p;
      } else if (vb == 2) {
        w[0] = *(const uint16_t *)p;
      } else {
        w[0] = *(const uint8_t *)p;
      }
    }
    // two channels at a time: a spekle step draws its normals in pairs
    for (int c = 0; c < nc; c += 2) {
      const bool two = c + 1 < nc;
      const int k0 = J.chan[c], k1 = two ? J.chan[c + 1] : k0;
      double v0, v1;
      int s0 = 0;
      if (!ROT || inside) {
        v0 = (double)(vec ? aug_elem<ES>(w, k0) : (uint32_t)src[(size_t)voff * C + k0]) * scale;   // exact
        v1 = (double)(vec ? aug_elem<ES>(w, k1) : (uint32_t)src[(size_t)voff * C + k1]) * scale;
      } else {   // outside the rotated source: 0.0 as of step fill_after
        v0 = v1 = 0.0;
        s0 = J.fill_after;
      }
      for (int s = s0; s < nsteps; ++s) {
        const hcu_aug_step &S = J.steps[s];
        const int c1 = two ? c + 1 : c;
        if (S.kind == HCU_AUG_SPEKLE) {
          double n0, n1;
          aug_normal2(S.key, (uint32_t)job, (uint32_t)s, ovox, (uint32_t)(c >> 1), n0, n1);
          v0 = aug_add_noise(v0, S.a[c], n0);
          v1 = aug_add_noise(v1, S.a[c1], n1);
        } else {
          v0 = aug_pointwise(S.kind, v0, S.a[c], S.b[c]);
          if (two) v1 = aug_pointwise(S.kind, v1, S.a[c1], S.b[c1]);
        }
      }
      uint16_t *row = tile + (c * kAugTX + xi) * pitch + yi * tz + zi;
      row[0] = d2h_rne((double)(float)v0);
      if (two) row[kAugTX * pitch] = d2h_rne((double)(float)v1);
    }
  }
  __syncthreads();
  // store: z fastest; for one (c, x) the tile's (y, z) rows are one contiguous
  // run of the destination when the tile spans the whole z extent
  uint16_t *dst = (uint16_t *)J.dst;
  if ((oz & 1) == 0 && ((uintptr_t)J.dst & 3) == 0) {   // even runs at even offsets: two halves per store
    const int hz = tz >> 1, n = nc * kAugTX * ty * hz;
    for (int i = tid; i < n; i += 256) {
      const int zi = (i % hz) * 2;
      int r = i / hz;
      const int yi = r % ty;
      r /= ty;
      const int xi = r & (kAugTX - 1), c = r >> 5;
      if (xi >= nx || yi >= ny || zi >= nz) continue;
      const uint32_t o = (((uint32_t)c * ox + xb + xi) * oy + yb + yi) * oz + zb + zi;
      *(uint32_t *)(dst + o) = *(const uint32_t *)(tile + (c * kAugTX + xi) * pitch + yi * tz + zi);
    }
  } else {
    const int n = nc * kAugTX * ty * tz;
    for (int i = tid; i < n; i += 256) {
      const int zi = i % tz;
      int r = i / tz;
      const int yi = r % ty;
      r /= ty;
      const int xi = r & (kAugTX - 1), c = r >> 5;
      if (xi >= nx || yi >= ny || zi >= nz) continue;
      const uint32_t o = (((uint32_t)c * ox + xb + xi) * oy + yb + yi) * oz + zb + zi;
      dst[o] = tile[(c * kAugTX + xi) * pitch + yi * tz + zi];
    }
  }
}

__global__ void __launch_bounds__(256) ingest_jobs_kernel(const hcu_ingest_job *jobs, int n_jobs) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kAugLds];
  int t = blockIdx.x, j = 0;
  AugTiling jt = aug_tiling(jobs[0].n_chan, jobs[0].ox, jobs[0].oy, jobs[0].oz);
  while (t >= jt.tiles && j + 1 < n_jobs) {
    t -= jt.tiles;
    ++j;
    jt = aug_tiling(jobs[j].n_chan, jobs[j].ox, jobs[j].oy, jobs[j].oz);
  }
  if (t >= jt.tiles) return;   // (the grid is the sum of the jobs' tiles)
  const hcu_ingest_job &J = jobs[j];
  if (J.rot) {
    if (J.src_dtype == HCU_U16)
      aug_job_tile<uint16_t, true>(J, jt, j, t, tile);
    else
      aug_job_tile<uint8_t, true>(J, jt, j, t, tile);
  } else if (J.src_dtype == HCU_U16) {
    aug_job_tile<uint16_t, false>(J, jt, j, t, tile);
  } else {
    aug_job_tile<uint8_t, false>(J, jt, j, t, tile);
  }
}

static bool aug_map_ok(const int *m, int n, int limit) {
  for (int i = 0; i < n; ++i)
    if (m[i] < 0 || m[i] >= limit) return false;
  return true;
}

// Everything the kernel relies on, checked from the host table before a launch.
static int aug_validate(const hcu_ingest_job &J, int idx) {
  const std::string at = "ingest_jobs: job " + std::to_string(idx) + ": ";
  if (!J.src || !J.dst) return fail(HCU_ERR_INVALID, at + "null src / dst");
  if (J.src_dtype != HCU_U16 && J.src_dtype != HCU_U8)
    return fail(HCU_ERR_INVALID, at + "Expected image datatype of uint8 or uint16");
  if (J.C > HCU_INGEST_MAX_C || J.n_chan > HCU_INGEST_MAX_C)
    return fail(HCU_ERR_UNSUPPORTED, at + "more than 16 channels");
  if (J.n_steps > HCU_AUG_MAX_STEPS) return fail(HCU_ERR_UNSUPPORTED, at + "more than 8 steps");
  if (J.Z <= 0 || J.Y <= 0 || J.X <= 0 || J.C <= 0) return fail(HCU_ERR_SHAPE, at + "empty source");
  if (J.ox <= 0 || J.oy <= 0 || J.oz <= 0 || J.n_chan <= 0) return fail(HCU_ERR_SHAPE, at + "empty extent");
  if (J.n_steps < 0) return fail(HCU_ERR_INVALID, at + "negative step count");
  const int es = J.src_dtype == HCU_U16 ? 2 : 1;
  if ((int64_t)J.Z * J.Y * J.X * J.C * es >= (1ll << 31))
    return fail(HCU_ERR_UNSUPPORTED, at + "source of 2^31 bytes or more");
  if ((int64_t)J.n_chan * J.ox * J.oy * J.oz >= (1ll << 31))
    return fail(HCU_ERR_UNSUPPORTED, at + "destination of 2^31 elements or more");
  if (((uintptr_t)J.src % es) || ((uintptr_t)J.dst % 2)) return fail(HCU_ERR_INVALID, at + "misaligned src / dst");
  if (J.z0 < 0 || (int64_t)J.z0 + J.oz > J.Z) return fail(HCU_ERR_SHAPE, at + "z window outside the source");
  if ((J.xmap_dev == nullptr) != (J.xmap_host == nullptr) || (J.ymap_dev == nullptr) != (J.ymap_host == nullptr))
    return fail(HCU_ERR_INVALID, at + "an index map needs its device and its host copy");
  if (J.rot != 0 && J.rot != 1) return fail(HCU_ERR_INVALID, at + "rot must be 0 or 1");
  int vx = J.ox, vy = J.oy;   // extents of the view the window / maps describe: the pre-rotation view with rot
  if (J.rot) {
    for (int i = 0; i < 4; ++i)
      if (!(std::fabs(J.rot_m[i]) <= 1.0)) return fail(HCU_ERR_INVALID, at + "rotation matrix entry not in [-1, 1]");
    if (!std::isfinite(J.rot_off[0]) || !std::isfinite(J.rot_off[1]))
      return fail(HCU_ERR_INVALID, at + "rotation offset not finite");
    if (J.rot_nx <= 0 || J.rot_ny <= 0) return fail(HCU_ERR_SHAPE, at + "empty pre-rotation view");
    if (J.rot_px < 0 || (int64_t)J.rot_px + J.ox > J.rot_nx || J.rot_py < 0 || (int64_t)J.rot_py + J.oy > J.rot_ny)
      return fail(HCU_ERR_SHAPE, at + "output window outside the rotated view");
    if (J.fill_after < 0 || J.fill_after > J.n_steps)
      return fail(HCU_ERR_INVALID, at + "fill_after outside [0, n_steps]");
    vx = J.rot_nx;
    vy = J.rot_ny;
  } else {
    bool zero = J.rot_nx == 0 && J.rot_ny == 0 && J.rot_px == 0 && J.rot_py == 0 && J.fill_after == 0 &&
                J.rot_off[0] == 0 && J.rot_off[1] == 0;   // (NaN != 0)
    for (int i = 0; i < 4; ++i) zero = zero && J.rot_m[i] == 0;
    if (!zero) return fail(HCU_ERR_INVALID, at + "rotation fields set without rot");
  }
  if (J.xmap_host ? !aug_map_ok(J.xmap_host, vx, J.X) : (J.x0 < 0 || (int64_t)J.x0 + vx > J.X))
    return fail(HCU_ERR_SHAPE, at + "x window or map entry outside the source");
  if (J.ymap_host ? !aug_map_ok(J.ymap_host, vy, J.Y) : (J.y0 < 0 || (int64_t)J.y0 + vy > J.Y))
    return fail(HCU_ERR_SHAPE, at + "y window or map entry outside the source");
  if (((uintptr_t)J.xmap_dev % 4) || ((uintptr_t)J.ymap_dev % 4)) return fail(HCU_ERR_INVALID, at + "misaligned map");
  for (int c = 0; c < J.n_chan; ++c)
    if (J.chan[c] < 0 || J.chan[c] >= J.C) return fail(HCU_ERR_INVALID, at + "channel index outside the source");
  for (int s = 0; s < J.n_steps; ++s)
    if (J.steps[s].kind < HCU_AUG_NORMALIZE || J.steps[s].kind > HCU_AUG_SPEKLE)
      return fail(HCU_ERR_INVALID, at + "unknown step kind");
  return 0;
}

}  // namespace hcu

using namespace hcu;

extern "C" int hcu_ingest_jobs(const hcu_ingest_job *jobs_host, const hcu_ingest_job *jobs_dev, int n_jobs,
                               hcu_stream_t stream) {
  if (!jobs_host || !jobs_dev) return fail(HCU_ERR_INVALID, "ingest_jobs: null job table");
  if (n_jobs <= 0) return fail(HCU_ERR_SHAPE, "ingest_jobs: no jobs");
  int64_t tiles = 0;
  double bytes = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const hcu_ingest_job &J = jobs_host[j];
    if (const int rc = aug_validate(J, j)) return rc;
    tiles += aug_tiling(J.n_chan, J.ox, J.oy, J.oz).tiles;
    // (a rotated job gathers at most one source voxel per output voxel: its reads count as its outputs)
    bytes += (double)J.ox * J.oy * J.oz * (J.C * (J.src_dtype == HCU_U16 ? 2 : 1) + J.n_chan * 2);
  }
  if (tiles > 0x7fffffff) return fail(HCU_ERR_UNSUPPORTED, "ingest_jobs: too many tiles");
  hipStream_t s = (hipStream_t)stream;
  HCU_TIMED(s, "ingest_jobs_kernel", 0.0, bytes,
            HCU_LAUNCH(ingest_jobs_kernel, dim3((unsigned)tiles), dim3(256), 0, s, jobs_dev, n_jobs));
  HCU_CHECK_LAUNCH();
  return 0;
}
