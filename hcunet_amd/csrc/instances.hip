// Instance labels from RDCNet's vector field (the reference's
// hcat/segment.py, which runs as numpy / numba / scipy on the host):
//   hcu_vec_votes        hist3d's counting loop (:640-656) for every voxel
//   hcu_vote_hist        hist3d's normalisation (:658)
//   hcu_vote_smooth      maximum_filter(size=2) and gaussian(sigma) (:602-603)
//   hcu_smooth_f64       the Gaussian alone
//   hcu_peak_candidates  the local-maximum test of peak_local_max (:605)
//   hcu_vec_label        nearest peak of every voxel's vote, masked (:609-626)
//   hcu_vec_label_paste  the same winner for one window of a tiled stack, renumbered to a
//                        stack-wide id and written into the stack's int32 label volume
// Volumes are [X][Y][Z] with Z contiguous; consecutive lanes run along Z.
// Votes and the candidate list use integer atomics only (exact, order-free);
// the float work is one IEEE division of exact integers, fp64 multiply / add
// in scipy's order and fp32 multiply / add / square root in numpy's, all
// under `fp contract(off)`: the build's default would fuse a multiply-add and
// round once where the reference rounds twice.
//
// The Gaussian: one kernel for all three axes over the view [outer][L][inner]
// (axis 0: 1, X, Y*Z; axis 1: X, Y, Z; axis 2: X*Y, Z, 1).  A workgroup owns
// TO lines x TL positions x IC inner elements and stages them, with up to 20
// positions of halo on each side that exist in the volume, in LDS (at most
// 3328 doubles = 26 KB); edge clamping happens on the LDS index.  Slab loads
// and output stores walk the inner axis first, so the X and Y passes read and
// write runs of IC * 8 contiguous bytes and the Z pass whole lines; LDS reads
// of a wave are consecutive doubles.  The first pass builds its slab from the
// integer counts: maximum over the offsets {-1,0}^3 inside the volume
// (outside is 0 and never wins), then (1 + m) / (1 + max count), the maximum
// commuting with the monotone normalisation.
#include <cmath>

#include "common.h"
#include "timing.h"
#include "hcunet.h"

namespace hcu {

constexpr int kSmoothSlab = 3328;          // doubles of LDS per workgroup
constexpr int kSmoothOut = 2048;           // outputs per workgroup (at most)
constexpr float kFarthest = 100000.0f;     // min_dist's initial value (:610)
constexpr int kVoteSlots = 1024;           // a workgroup's LDS vote table (8 KB)
constexpr int kVoteProbes = 8;             // slots tried before a vote goes straight to global memory
constexpr uint32_t kVoteChunk = 4096;      // voxels per workgroup (at least)
constexpr uint32_t kNoVoxel = 0xFFFFFFFFu; // (a voxel index is below 2^31)
constexpr int kPeakSlots = 1024;           // peaks a workgroup of the paste pass keeps in LDS (16 KB)

struct alignas(16) PeakSlot {
  float p0, p1, p2;   // the peak, as the distance reads it
  int32_t id;         // its stack-wide id, 0: not this window's
};
struct VoteBounds {
  float lo[3], hi[3];   // floor(c) must lie in [lo, hi) on every axis
};

struct SmoothTaps {
  double w[HCU_VOTE_RADIUS + 1];   // w[k]: the tap at distance k
};
struct SmoothGeom {
  int outer, L, inner;
  int TO, TL, IC;      // tile: lines, positions, inner elements
  int nIC, nLT;        // tiles along inner and L
  int radius;
};

__device__ __forceinline__ float load_as_float(const void *p, int dtype, size_t i) {
  switch (dtype) {   // (uniform)
    case HCU_F32: return static_cast<const float *>(p)[i];
    case HCU_F16: return (float)static_cast<const _Float16 *>(p)[i];
    case HCU_BF16: return bf2f(static_cast<const uint16_t *>(p)[i]);
    case HCU_F64: return (float)static_cast<const double *>(p)[i];
    default: return (float)static_cast<const uint8_t *>(p)[i];
  }
}

// c = (x + v2, y + v1, z + v0) in fp32 (:590-593)
__device__ __forceinline__ void vote_of(const void *vec, int dtype, int64_t cs, uint32_t i, int x, int y,
                                        int z, float &c0, float &c1, float &c2) {
  c0 = (float)x + load_as_float(vec, dtype, (size_t)(2 * cs) + i);
  c1 = (float)y + load_as_float(vec, dtype, (size_t)cs + i);
  c2 = (float)z + load_as_float(vec, dtype, i);
}

__global__ void __launch_bounds__(256)
vec_votes_kernel(const void *vec, int dtype, int64_t cs, int points, uint32_t nvox, uint32_t chunk, FastDiv fZ,
                 FastDiv fY, int X, int Y, int Z, uint32_t *counts, uint32_t *max_count) {
  // Neighbouring voxels point at the same few voxels, and a voxel near a cell's centre receives
  // thousands of votes: sent one by one they queue on one address of L2.  A workgroup owns
  // `chunk` consecutive voxels and gathers their votes in an LDS table keyed by the voted voxel
  // (open addressing, a bounded probe, a full table falls through to global memory), then adds
  // each slot to the volume once.  Sums of integers: the order changes nothing.
  __shared__ uint32_t slot_key[kVoteSlots];
  __shared__ uint32_t slot_votes[kVoteSlots];
  for (int k = threadIdx.x; k < kVoteSlots; k += 256) {
    slot_key[k] = kNoVoxel;
    slot_votes[k] = 0;
  }
  __syncthreads();
  uint32_t top = 0;
  const uint32_t begin = blockIdx.x * chunk, end = begin + chunk < nvox ? begin + chunk : nvox;
  for (uint32_t i = begin + threadIdx.x; i < end; i += 256u) {
    int q, x, y, z;
    fZ.divmod(i, q, z);
    fY.divmod((uint32_t)q, x, y);
    float c0, c1, c2;
    if (points) {   // (uniform) hist3d: the planes are c0, c1, c2
      c0 = load_as_float(vec, dtype, i);
      c1 = load_as_float(vec, dtype, (size_t)cs + i);
      c2 = load_as_float(vec, dtype, (size_t)(2 * cs) + i);
    } else {
      vote_of(vec, dtype, cs, i, x, y, z, c0, c1, c2);
    }
    const float f0 = floorf(c0), f1 = floorf(c1), f2 = floorf(c2);
    // compared as floats, before any conversion: NaN and Inf fail, and no address is formed from them
    if (f0 >= 0.0f && f0 < (float)X && f1 >= 0.0f && f1 < (float)Y && f2 >= 0.0f && f2 < (float)Z) {
      const uint32_t at = ((uint32_t)(int)f0 * (uint32_t)Y + (uint32_t)(int)f1) * (uint32_t)Z + (uint32_t)(int)f2;
      bool held = false;
      const uint32_t h = (at * 2654435761u) >> 22;
      for (int p = 0; p < kVoteProbes && !held; ++p) {
        const uint32_t k = (h + (uint32_t)p) & (uint32_t)(kVoteSlots - 1);
        const uint32_t was = atomicCAS(&slot_key[k], kNoVoxel, at);
        if (was == kNoVoxel || was == at) {
          atomicAdd(&slot_votes[k], 1u);
          held = true;
        }
      }
      if (!held) {
        const uint32_t now = atomicAdd(counts + at, 1u) + 1u;
        top = now > top ? now : top;   // the last addition to the fullest voxel sees its final count
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kVoteSlots; k += 256) {
    const uint32_t at = slot_key[k], votes = slot_votes[k];
    if (at != kNoVoxel && votes) {
      const uint32_t now = atomicAdd(counts + at, votes) + votes;
      top = now > top ? now : top;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)top, off);
    top = o > top ? o : top;
  }
  if ((threadIdx.x & 63) == 0 && top) atomicMax(max_count, top);
}

__global__ void __launch_bounds__(256)
vote_hist_kernel(const uint32_t *counts, const uint32_t *max_count, uint32_t nvox, double *hist) {
  const double denom = 1.0 + (double)max_count[0];
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u)
    hist[i] = (1.0 + (double)counts[i]) / denom;
}

template <bool FUSED>
__global__ void __launch_bounds__(256)
smooth_pass_kernel(const double *in, const uint32_t *counts, const uint32_t *max_count, int Y, int Z,
                   const SmoothGeom g, const SmoothTaps taps, double *out) {
#pragma clang fp contract(off)
  __shared__ double slab[kSmoothSlab];
  const int tid = threadIdx.x, r = g.radius;
  uint32_t b = blockIdx.x;
  const int ic = (int)(b % (uint32_t)g.nIC);
  b /= (uint32_t)g.nIC;
  const int lt = (int)(b % (uint32_t)g.nLT), ot = (int)(b / (uint32_t)g.nLT);
  const int i0 = ic * g.IC, icw = min(g.IC, g.inner - i0);
  const int l0 = lt * g.TL, tl = min(g.TL, g.L - l0);
  const int o0 = ot * g.TO, to = min(g.TO, g.outer - o0);
  const int s0 = max(l0 - r, 0), sr = min(l0 + tl + r, g.L) - s0;   // slab rows: positions [s0, s0 + sr)
  const int nslab = to * sr * icw;
  double denom = 1.0;
  if (FUSED) denom = 1.0 + (double)max_count[0];
  for (int e = tid; e < nslab; e += 256) {
    const int q = e / icw, i = e - q * icw;
    const int o = q / sr, rr = q - o * sr;
    const size_t at = ((size_t)(o0 + o) * g.L + (size_t)(s0 + rr)) * g.inner + (size_t)(i0 + i);
    if (FUSED) {   // (outer is 1, inner is Y * Z)
      const int x = s0 + rr, yz = i0 + i, y = yz / Z, z = yz - y * Z;
      uint32_t m = 0;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int dx = n >> 2, dy = (n >> 1) & 1, dz = n & 1;
        if (x >= dx && y >= dy && z >= dz) {
          const uint32_t c = counts[at - (size_t)dx * g.inner - (size_t)(dy * Z + dz)];
          m = c > m ? c : m;
        }
      }
      slab[e] = (1.0 + (double)m) / denom;
    } else {
      slab[e] = in[at];
    }
  }
  __syncthreads();
  const int nout = to * tl * icw;
  for (int e = tid; e < nout; e += 256) {
    const int q = e / icw, i = e - q * icw;
    const int o = q / tl, t = q - o * tl;
    const int l = l0 + t;
    const double *col = slab + o * sr * icw + i;   // position p of this line: col[(p - s0) * icw]
    double acc = col[(l - s0) * icw] * taps.w[0];
    for (int k = r; k >= 1; --k) {
      const int lo = max(l - k, 0) - s0, hi = min(l + k, g.L - 1) - s0;
      acc = acc + (col[lo * icw] + col[hi * icw]) * taps.w[k];
    }
    out[((size_t)(o0 + o) * g.L + (size_t)l) * g.inner + (size_t)(i0 + i)] = acc;
  }
}

// doubles <-> 64-bit keys whose unsigned order is the numeric order
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__global__ void __launch_bounds__(256)
volume_min_kernel(const double *h, uint32_t nvox, unsigned long long *min_key) {
  unsigned long long low = ~0ull;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    const unsigned long long k = order_key(h[i]);
    low = k < low ? k : low;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)low, off);
    low = o < low ? o : low;
  }
  if ((threadIdx.x & 63) == 0) atomicMin(min_key, low);
}

__global__ void __launch_bounds__(256)
peak_candidates_kernel(const double *h, uint32_t nvox, FastDiv fZ, FastDiv fY, int X, int Y, int Z,
                       const unsigned long long *min_key, int32_t *cand_index, double *cand_value,
                       int capacity, int *count) {
  const double lowest = key_value(min_key[0]);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    int q, x, y, z;
    fZ.divmod(i, q, z);
    fY.divmod((uint32_t)q, x, y);
    // off the outermost layers: the whole 3x3x3 neighbourhood lies inside the volume
    if (x < 1 || x > X - 2 || y < 1 || y > Y - 2 || z < 1 || z > Z - 2) continue;
    const double v = h[i];
    if (!(v > lowest)) continue;
    bool top = true;
    for (int dx = -1; dx <= 1 && top; ++dx)
      for (int dy = -1; dy <= 1; ++dy) {
        const double *row = h + ((size_t)(x + dx) * Y + (size_t)(y + dy)) * Z + z;
        top = top && row[-1] <= v && row[0] <= v && row[1] <= v;
      }
    if (top) {
      const int slot = atomicAdd(count, 1);
      if (slot < capacity) {
        cand_index[slot] = (int32_t)i;
        cand_value[slot] = v;
      }
    }
  }
}

__global__ void __launch_bounds__(256)
vec_label_kernel(const void *vec, int dtype, int64_t cs, uint32_t nvox, FastDiv fZ, FastDiv fY,
                 const int32_t *__restrict__ peaks, int n, const void *mask, int mask_dtype, int label_offset,
                 double *label) {
#pragma clang fp contract(off)
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    int q, x, y, z;
    fZ.divmod(i, q, z);
    fY.divmod((uint32_t)q, x, y);
    float c0, c1, c2;
    vote_of(vec, dtype, cs, i, x, y, z, c0, c1, c2);
    float nearest = kFarthest;
    int won = -label_offset;   // nothing below 100000: the label stays 0
    for (int k = 0; k < n; ++k) {   // (uniform index: every lane reads the same peak)
      const float d0 = c0 - (float)peaks[3 * k], d1 = c1 - (float)peaks[3 * k + 1],
                  d2 = c2 - (float)peaks[3 * k + 2];
      const float d = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
      if (nearest > d) {   // strict, and false for a NaN distance
        nearest = d;
        won = k;
      }
    }
    if (mask && load_as_float(mask, mask_dtype, i) < 0.2f) won = -label_offset;
    label[i] = (double)(won + label_offset);
  }
}

// vec_label_kernel's winner per voxel of one window of a larger volume, renumbered through `ids` and
// written into that volume at the window's origin.  A voxel is written only where a peak won, its id
// is not 0, the mask keeps it and floor(c) lies inside the vote bounds; every other destination voxel
// is left as it was.  The first kPeakSlots peaks are staged once per workgroup as floats next to
// their ids (one 16-byte LDS read per peak, the same address in every lane); any further ones are read
// from global memory at a wave-uniform index.  (float)peak is exact either way: same bits.
__global__ void __launch_bounds__(256)
vec_label_paste_kernel(const void *vec, int dtype, int64_t cs, uint32_t nvox, FastDiv fZ, FastDiv fY,
                       const int32_t *__restrict__ peaks, const int32_t *__restrict__ ids, int n, const void *mask,
                       int mask_dtype, const VoteBounds vb, int32_t *dst, int DY, int DZ, int ox, int oy, int oz) {
#pragma clang fp contract(off)
  __shared__ PeakSlot table[kPeakSlots];
  const int staged = n < kPeakSlots ? n : kPeakSlots;
  for (int k = threadIdx.x; k < staged; k += 256) {
    PeakSlot p;
    p.p0 = (float)peaks[3 * k];
    p.p1 = (float)peaks[3 * k + 1];
    p.p2 = (float)peaks[3 * k + 2];
    p.id = ids[k];
    table[k] = p;
  }
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
    int q, x, y, z;
    fZ.divmod(i, q, z);
    fY.divmod((uint32_t)q, x, y);
    float c0, c1, c2;
    vote_of(vec, dtype, cs, i, x, y, z, c0, c1, c2);
    float nearest = kFarthest;
    int id = 0;   // nothing below 100000, or a winner that another window owns: no write
    for (int k = 0; k < staged; ++k) {
      const PeakSlot p = table[k];
      const float d0 = c0 - p.p0, d1 = c1 - p.p1, d2 = c2 - p.p2;
      const float d = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
      if (nearest > d) {   // strict, and false for a NaN distance
        nearest = d;
        id = p.id;
      }
    }
    for (int k = staged; k < n; ++k) {   // (uniform index: every lane reads the same peak)
      const float d0 = c0 - (float)peaks[3 * k], d1 = c1 - (float)peaks[3 * k + 1],
                  d2 = c2 - (float)peaks[3 * k + 2];
      const float d = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
      if (nearest > d) {
        nearest = d;
        id = ids[k];
      }
    }
    if (id == 0) continue;
    if (mask && load_as_float(mask, mask_dtype, i) < 0.2f) continue;
    const float f0 = floorf(c0), f1 = floorf(c1), f2 = floorf(c2);
    // compared as floats against bounds that may be +-Inf; a NaN or Inf vote has no winner above
    if (!(f0 >= vb.lo[0] && f0 < vb.hi[0] && f1 >= vb.lo[1] && f1 < vb.hi[1] && f2 >= vb.lo[2] && f2 < vb.hi[2]))
      continue;
    dst[((size_t)(ox + x) * (size_t)DY + (size_t)(oy + y)) * (size_t)DZ + (size_t)(oz + z)] = id;
  }
}

static int volume_voxels(const char *what, int X, int Y, int Z, uint32_t *nvox) {
  if (X <= 0 || Y <= 0 || Z <= 0) return fail(HCU_ERR_SHAPE, std::string(what) + ": empty volume");
  const int64_t n = (int64_t)X * Y * Z;
  if (n >= (1ll << 31)) return fail(HCU_ERR_UNSUPPORTED, std::string(what) + ": X*Y*Z must be below 2^31");
  *nvox = (uint32_t)n;
  return 0;
}
static int vector_ok(const char *what, const void *vec, int dtype, int64_t chan_stride, uint32_t nvox) {
  if (!vec) return fail(HCU_ERR_INVALID, std::string(what) + ": null argument");
  if (dtype != HCU_F32 && dtype != HCU_F16 && dtype != HCU_BF16)
    return fail(HCU_ERR_INVALID, std::string(what) + ": the vector field is fp32, fp16 or bf16");
  if (chan_stride < (int64_t)nvox)
    return fail(HCU_ERR_INVALID, std::string(what) + ": chan_stride below X*Y*Z, the channel planes overlap");
  return 0;
}
static int voxel_grid(uint32_t nvox) { return (int)std::min<uint32_t>((nvox + 255u) / 256u, 4096u); }

static SmoothGeom smooth_geom(int outer, int L, int inner, int radius) {
  SmoothGeom g{};
  g.outer = outer;
  g.L = L;
  g.inner = inner;
  g.radius = radius;
  g.IC = std::min(inner, 32);
  g.TL = std::min(L, 64);
  g.TO = std::max(1, std::min(outer, kSmoothOut / (g.TL * g.IC)));
  g.nIC = cdiv(inner, g.IC);
  g.nLT = cdiv(L, g.TL);
  return g;
}
// rows of a slab are at most TL + 2 * radius, and at most L
static bool smooth_fits(const SmoothGeom &g) {
  return (int64_t)g.TO * std::min(g.TL + 2 * g.radius, g.L) * g.IC <= kSmoothSlab;
}

static int smooth_taps(const char *what, const double *weights, int radius, SmoothTaps *taps) {
  if (!weights) return fail(HCU_ERR_INVALID, std::string(what) + ": null argument");
  if (radius < 0 || radius > HCU_VOTE_RADIUS)
    return fail(HCU_ERR_INVALID, std::string(what) + ": radius outside [0, HCU_VOTE_RADIUS]");
  for (int k = 0; k <= HCU_VOTE_RADIUS; ++k) taps->w[k] = k <= radius ? weights[radius - k] : 0.0;
  return 0;
}

// The passes over axes 0, 1, 2: src (or the counts) -> a -> b -> a ... so that the last lands in out.
static int smooth_passes(const char *what, const double *in, const uint32_t *counts, const uint32_t *max_count,
                         int X, int Y, int Z, uint32_t nvox, const SmoothTaps &taps, int radius, double *out,
                         double *scratch, hipStream_t s) {
  const SmoothGeom geom[3] = {smooth_geom(1, X, Y * Z, radius), smooth_geom(X, Y, Z, radius),
                              smooth_geom(X * Y, Z, 1, radius)};
  int64_t blocks[3];
  for (int a = 0; a < 3; ++a) {
    const SmoothGeom &g = geom[a];
    blocks[a] = (int64_t)g.nIC * g.nLT * cdiv(g.outer, g.TO);
    if (!smooth_fits(g) || blocks[a] >= (1ll << 31))
      return fail(HCU_ERR_UNSUPPORTED, std::string(what) + ": no tiling for this volume");
  }
  const double bytes = (double)nvox * 16.0;
  double *dst[3] = {out, scratch, out};
  const double *src[3] = {in, out, scratch};
  if (counts) {
    HCU_TIMED(s, "smooth_pass_kernel<votes,x>", (double)nvox * (3.0 * radius + 2.0), (double)nvox * 12.0,
              HCU_LAUNCH(smooth_pass_kernel<true>, dim3((unsigned)blocks[0]), dim3(256), 0, s,
                         (const double *)nullptr, counts, max_count, Y, Z, geom[0], taps, dst[0]));
  } else {
    HCU_TIMED(s, "smooth_pass_kernel<x>", (double)nvox * (3.0 * radius + 1.0), bytes,
              HCU_LAUNCH(smooth_pass_kernel<false>, dim3((unsigned)blocks[0]), dim3(256), 0, s, src[0],
                         (const uint32_t *)nullptr, (const uint32_t *)nullptr, Y, Z, geom[0], taps, dst[0]));
  }
  HCU_TIMED(s, "smooth_pass_kernel<y>", (double)nvox * (3.0 * radius + 1.0), bytes,
            HCU_LAUNCH(smooth_pass_kernel<false>, dim3((unsigned)blocks[1]), dim3(256), 0, s, src[1],
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr, Y, Z, geom[1], taps, dst[1]));
  HCU_TIMED(s, "smooth_pass_kernel<z>", (double)nvox * (3.0 * radius + 1.0), bytes,
            HCU_LAUNCH(smooth_pass_kernel<false>, dim3((unsigned)blocks[2]), dim3(256), 0, s, src[2],
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr, Y, Z, geom[2], taps, dst[2]));
  HCU_CHECK_LAUNCH();
  return 0;
}

}  // namespace hcu

using namespace hcu;

extern "C" int hcu_vec_votes(const void *vec, int dtype, int64_t chan_stride, int points, int X, int Y, int Z,
                             uint32_t *counts, uint32_t *max_count, hcu_stream_t stream) {
  if (!counts || !max_count) return fail(HCU_ERR_INVALID, "vec_votes: null argument");
  uint32_t nvox;
  if (int rc = volume_voxels("vec_votes", X, Y, Z, &nvox)) return rc;
  if (int rc = vector_ok("vec_votes", vec, dtype, chan_stride, nvox)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == HCU_F32 ? 4.0 : 2.0;
  // workgroups of kVoteChunk voxels, or of more where that would be over 4096 workgroups
  const uint32_t chunk = std::max(kVoteChunk, ((nvox + 4095u) / 4096u + 255u) / 256u * 256u);
  HCU_TIMED(s, "vec_votes_kernel", 0.0, (double)nvox * (3.0 * es + 8.0),
            HCU_LAUNCH(vec_votes_kernel, dim3((nvox + chunk - 1) / chunk), dim3(256), 0, s, vec, dtype, chan_stride,
                       points != 0, nvox, chunk, FastDiv((uint32_t)Z), FastDiv((uint32_t)Y), X, Y, Z, counts,
                       max_count));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_vote_hist(const uint32_t *counts, const uint32_t *max_count, int X, int Y, int Z,
                             double *hist, hcu_stream_t stream) {
  if (!counts || !max_count || !hist) return fail(HCU_ERR_INVALID, "vote_hist: null argument");
  uint32_t nvox;
  if (int rc = volume_voxels("vote_hist", X, Y, Z, &nvox)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HCU_TIMED(s, "vote_hist_kernel", (double)nvox, (double)nvox * 12.0,
            HCU_LAUNCH(vote_hist_kernel, dim3(voxel_grid(nvox)), dim3(256), 0, s, counts, max_count, nvox, hist));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_vote_smooth(const uint32_t *counts, const uint32_t *max_count, int X, int Y, int Z,
                               const double *weights, int radius, double *out, double *scratch,
                               hcu_stream_t stream) {
  if (!counts || !max_count || !out || !scratch) return fail(HCU_ERR_INVALID, "vote_smooth: null argument");
  if (out == scratch) return fail(HCU_ERR_INVALID, "vote_smooth: out and scratch are the same buffer");
  uint32_t nvox;
  if (int rc = volume_voxels("vote_smooth", X, Y, Z, &nvox)) return rc;
  SmoothTaps taps;
  if (int rc = smooth_taps("vote_smooth", weights, radius, &taps)) return rc;
  return smooth_passes("vote_smooth", nullptr, counts, max_count, X, Y, Z, nvox, taps, radius, out, scratch,
                       (hipStream_t)stream);
}

extern "C" int hcu_smooth_f64(const double *in, int X, int Y, int Z, const double *weights, int radius,
                              double *out, double *scratch, hcu_stream_t stream) {
  if (!in || !out || !scratch) return fail(HCU_ERR_INVALID, "smooth_f64: null argument");
  if (out == scratch || in == out || in == scratch)
    return fail(HCU_ERR_INVALID, "smooth_f64: in, out and scratch must be distinct buffers");
  uint32_t nvox;
  if (int rc = volume_voxels("smooth_f64", X, Y, Z, &nvox)) return rc;
  SmoothTaps taps;
  if (int rc = smooth_taps("smooth_f64", weights, radius, &taps)) return rc;
  return smooth_passes("smooth_f64", in, nullptr, nullptr, X, Y, Z, nvox, taps, radius, out, scratch,
                       (hipStream_t)stream);
}

extern "C" int hcu_peak_candidates(const double *h, int X, int Y, int Z, int32_t *cand_index,
                                   double *cand_value, int capacity, uint32_t *state, int *n_found,
                                   hcu_stream_t stream) {
  if (!h || !cand_index || !cand_value || !state || !n_found)
    return fail(HCU_ERR_INVALID, "peak_candidates: null argument");
  if (capacity <= 0) return fail(HCU_ERR_INVALID, "peak_candidates: capacity must be positive");
  if ((uintptr_t)state % 8) return fail(HCU_ERR_INVALID, "peak_candidates: state must be 8-byte aligned");
  uint32_t nvox;
  if (int rc = volume_voxels("peak_candidates", X, Y, Z, &nvox)) return rc;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *min_key = (unsigned long long *)state;
  int *count = (int *)(state + 2);
  HCU_HIP(hipMemsetAsync(min_key, 0xFF, sizeof(unsigned long long), s));
  HCU_HIP(hipMemsetAsync(count, 0, 2 * sizeof(int), s));
  HCU_TIMED(s, "volume_min_kernel", 0.0, (double)nvox * 8.0,
            HCU_LAUNCH(volume_min_kernel, dim3(std::min(voxel_grid(nvox), 512)), dim3(256), 0, s, h, nvox, min_key));
  HCU_TIMED(s, "peak_candidates_kernel", 0.0, (double)nvox * 8.0,
            HCU_LAUNCH(peak_candidates_kernel, dim3(voxel_grid(nvox)), dim3(256), 0, s, h, nvox,
                       FastDiv((uint32_t)Z), FastDiv((uint32_t)Y), X, Y, Z, (const unsigned long long *)min_key,
                       cand_index, cand_value, capacity, count));
  HCU_CHECK_LAUNCH();
  int found = 0;
  HCU_HIP(hipMemcpyAsync(&found, count, sizeof(int), hipMemcpyDeviceToHost, s));
  HCU_HIP(hipStreamSynchronize(s));
  *n_found = found;
  if (found > capacity)
    return fail(HCU_ERR_WORKSPACE, "peak_candidates: " + std::to_string(found) + " candidates, room for " +
                                       std::to_string(capacity));
  return 0;
}

extern "C" int hcu_vec_label(const void *vec, int dtype, int64_t chan_stride, int X, int Y, int Z,
                             const int32_t *peaks, int n, const void *mask, int mask_dtype, int label_offset,
                             double *label, hcu_stream_t stream) {
  if (!label) return fail(HCU_ERR_INVALID, "vec_label: null argument");
  uint32_t nvox;
  if (int rc = volume_voxels("vec_label", X, Y, Z, &nvox)) return rc;
  if (int rc = vector_ok("vec_label", vec, dtype, chan_stride, nvox)) return rc;
  if (n < 0 || (n > 0 && !peaks)) return fail(HCU_ERR_INVALID, "vec_label: n peaks need a peak table");
  if (label_offset < 0 || label_offset > (1 << 20))
    return fail(HCU_ERR_INVALID, "vec_label: label_offset outside [0, 2^20]");
  if (mask && mask_dtype != HCU_U8 && mask_dtype != HCU_F32 && mask_dtype != HCU_F16 && mask_dtype != HCU_BF16 &&
      mask_dtype != HCU_F64)
    return fail(HCU_ERR_INVALID, "vec_label: the mask is uint8, fp32, fp16, bf16 or float64");
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == HCU_F32 ? 4.0 : 2.0;
  HCU_TIMED(s, "vec_label_kernel", (double)nvox * 9.0 * n, (double)nvox * (3.0 * es + 9.0),
            HCU_LAUNCH(vec_label_kernel, dim3(voxel_grid(nvox)), dim3(256), 0, s, vec, dtype, chan_stride, nvox,
                       FastDiv((uint32_t)Z), FastDiv((uint32_t)Y), peaks, n, mask, mask_dtype, label_offset,
                       label));
  HCU_CHECK_LAUNCH();
  return 0;
}

extern "C" int hcu_vec_label_paste(const void *vec, int dtype, int64_t chan_stride, int X, int Y, int Z,
                                   const int32_t *peaks, const int32_t *ids, int n, const void *mask,
                                   int mask_dtype, const float *bounds, int32_t *dst, int DX, int DY, int DZ,
                                   int ox, int oy, int oz, hcu_stream_t stream) {
  if (!dst || !bounds) return fail(HCU_ERR_INVALID, "vec_label_paste: null argument");
  uint32_t nvox, ndst;
  if (int rc = volume_voxels("vec_label_paste", X, Y, Z, &nvox)) return rc;
  if (int rc = volume_voxels("vec_label_paste destination", DX, DY, DZ, &ndst)) return rc;
  if (int rc = vector_ok("vec_label_paste", vec, dtype, chan_stride, nvox)) return rc;
  if (n < 0 || (n > 0 && (!peaks || !ids)))
    return fail(HCU_ERR_INVALID, "vec_label_paste: n peaks need a peak table and an id table");
  if (mask && mask_dtype != HCU_U8 && mask_dtype != HCU_F32 && mask_dtype != HCU_F16 && mask_dtype != HCU_BF16 &&
      mask_dtype != HCU_F64)
    return fail(HCU_ERR_INVALID, "vec_label_paste: the mask is uint8, fp32, fp16, bf16 or float64");
  VoteBounds vb;
  for (int a = 0; a < 3; ++a) {
    vb.lo[a] = bounds[2 * a];
    vb.hi[a] = bounds[2 * a + 1];
    if (std::isnan(vb.lo[a]) || std::isnan(vb.hi[a]))
      return fail(HCU_ERR_INVALID, "vec_label_paste: a vote bound is NaN");
  }
  if (ox < 0 || oy < 0 || oz < 0 || (int64_t)ox + X > DX || (int64_t)oy + Y > DY || (int64_t)oz + Z > DZ)
    return fail(HCU_ERR_SHAPE, "vec_label_paste: the window does not lie inside the destination");
  if (n == 0) return 0;   // no peak: nothing wins, nothing is written
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == HCU_F32 ? 4.0 : 2.0;
  HCU_TIMED(s, "vec_label_paste_kernel", (double)nvox * 9.0 * n, (double)nvox * (3.0 * es + 5.0),
            HCU_LAUNCH(vec_label_paste_kernel, dim3(voxel_grid(nvox)), dim3(256), 0, s, vec, dtype, chan_stride,
                       nvox, FastDiv((uint32_t)Z), FastDiv((uint32_t)Y), peaks, ids, n, mask, mask_dtype, vb, dst,
                       DY, DZ, ox, oy, oz));
  HCU_CHECK_LAUNCH();
  return 0;
}
