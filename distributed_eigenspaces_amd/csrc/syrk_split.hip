// Covariance SYRK on CDNA4 bf16 MFMA with split fp32 operands ("split3"):
//   S = alpha * X^T X  (+ S if accumulating),  X: n x d fp32 row-major.
//
// Replaces SlaveNode.compute_sigma_hat_ (distributed.py:59-70; np.dot(x.T, x)
// on a transposed view -> OpenBLAS dsyrk, then /= n).  gfx950 has no xf32 MFMA
// and its f32 MFMA runs at 1/16 of the bf16 rate, so every fp32 sample is split
// once into x = hi + lo (hi = bf16(x), lo = bf16(x - hi); |x - hi - lo| <=
// 2^-17 |x|) and each product is formed from three bf16 MFMA products
//   x_a x_b ~ hi_a hi_b + hi_a lo_b + lo_a hi_b
// accumulated in fp32 (the bf16 products are exact in fp32).  The dropped
// lo_a lo_b term is ~2^-18 |x_a x_b|: negligible off the diagonal (zero-mean
// rounding residues), but it biases the diagonal by ~-3e-6 relative, so the
// split pass also accumulates sum_k lo_ik^2 per feature and a last kernel adds it
// to S[i][i].  Net error vs float64 ~1e-7 * max|S|, the same order as the
// fp32-MFMA kernel (syrk.hip), at 16/3 x its MFMA rate.
//
// Two paths by width (kFusedMaxD below, with the measurements behind it):
//  d <= 2048: syrks_kernel, persistent, one 512-thread block per CU, stages X as it
//   lies in HBM (fp32 rows) and splits it in LDS - no image, one pass over all rows -
//   then syrks_reduce_kernel and diag_corr_kernel as below;
//  d > 2048, per row chunk (bounded workspace; chunks accumulate into S):
//   split_kernel   X (fp32, HBM) -> XP: bf16 hi/lo image in MFMA operand order,
//                  [32-row block][256-feature panel][slice = (octet, hi|lo)]
//                  [feature][8 rows] - a panel's K-tile is 32 contiguous KiB -
//                  rows padded with zeros to a multiple of 32, + lo^2 partials;
//   syrks_h_kernel persistent, one 512-thread block per CU, 256 x 256 lower
//                  tiles, v_mfma_f32_16x16x32_bf16, K-tile = 32 rows whose two
//                  panels (32 KiB each: 4 octets x {hi, lo} x 256 features x 16 B)
//                  are DMA'd L2/HBM -> LDS with buffer_load ... lds into two
//                  ring buffers restaged half a K-tile at a time (segment_h: 2
//                  phases per K-tile, waves 4-7 one barrier behind, counted
//                  vmcnt + raw s_barrier); conflict-free ds_read_b128 reads;
//                  diagonal tiles read their B operands from the A quarters and skip
//                  the MFMA blocks above the diagonal;
//   syrks_reduce_kernel  split-K remainder tiles, summed in block order (deterministic);
//   diag_corr_kernel  S[i][i] += alpha * sum lo_i^2.
// Tile order: compact XCD groups where G = 256 and nt % 8 == 0
// (tile_order_compact_kernel), else 8 x 4 super-tiles of the lower triangle, so the
// ~32 tiles an XCD runs concurrently share few panels in its L2.
// The two persistent kernels differ only in how a K-tile reaches LDS and how the MFMA
// phases are ordered (segment, segment_h); around the K loop both are the same, each
// piece stated once:
//  work_item    the schedule (no atomics): q = T / G full phases of one tile per block;
//               the R = T mod G remainder tiles are cut into nseg equal K segments run
//               K-synchronously (segment-major item order) and summed in segment order
//               by syrks_reduce.  One WorkItem = tile, K range, slab slot, pacing sequence;
//  pace_point   the item's PaceSeq: every pace_kt K-tiles the XCD's blocks (and every
//               other time all blocks) wait for each other;
//  tile_ctx / finish_tile   the wave's place in the tile and its slab; after the K loop
//               the flushed sums are added back and the tile goes to S or to its slab;
//  run_pass     (host) pacing counters, kernel, syrks_reduce, diag_corr - once for the
//               fused path, once per row chunk above it.
#include <cmath>
#include <cstdlib>

#include "bf16_split.hpp"
#include "deig_internal.hpp"
#include "lds_dma.hpp"

namespace deig {
namespace {

constexpr int BT = 256;                      // tile edge (features)
constexpr int ROWS_PAD = 32;                 // chunk rows are padded to this (2 k-steps)
constexpr int NTHR = 512;                    // 8 waves: 2 (i) x 4 (j), wave tile 128 x 64
constexpr int SLICE_B = BT * 16;             // (octet, hi|lo) slice of a panel: 4 KiB
constexpr int SLAB = BT * BT;                // floats per partial slab
constexpr int SPLIT_YB = 256;                // row groups of the split pass
constexpr int SUPER_H = 8, SUPER_W = 4;      // super-tile shape (tiles)
constexpr int BLOCK_B = 8 * SLICE_B;         // one panel of a 32-row block: 32 KiB
// Recommended XP image per chunk: a config-3 shard (2^21 x 8192) in one chunk on
// a 288 GB MI355X; callers with less room pass a smaller workspace and get chunks.
constexpr size_t DEFAULT_CHUNK_BYTES = size_t(64) << 30;

struct SSched {
  unsigned char* XP;  // bf16 image of this chunk (split_kernel writes, syrks_h_kernel reads)
  float* S;
  float* part;   // one slab per remainder item
  float* accs;   // 1 flush slab per block
  const int* order;  // tile order: ti | tj << 16
  int64_t lds, dp;
  int64_t NK;  // K-tiles in the chunk
  int nseg;    // K segments per remainder tile (items = R * nseg)
  int d, nt, T, G, q, R;
  float alpha;
  int beta;
  int flush_kt;  // K-tiles between two-level flushes of the accumulators
  unsigned* pace;  // per-XCD arrival counters (128 B apart), zeroed per launch
  int pace_kt;     // K-tiles between two XCD pacing points (0: off)
  // fused split: X is staged as fp32 and split in LDS
  const float* X;
  int64_t ldx, nrows;
  float* corr;  // lo^2 partials: [segment][octet wave][dp]
};

// XCD pacing point of the full-tile phases: the ~G/8 blocks on one XCD run
// neighbouring tiles of one super-tile and read the same K rows of its panels, but
// drift apart over ~10^5 K-tiles until their shared panels no longer meet in the
// XCD's 4 MB L2.  Every pace_kt K-tiles one lane per block adds 1 to its XCD's
// counter and waits (bounded: 20 us of s_memrealtime, so a block that is not
// resident can only cost time, never a hang) until all of the XCD's blocks have
// arrived.  Relaxed atomics, no fence: nothing is published, so no L2 write-back.
// The result's wait (vmcnt(0)) also drains this wave's ring DMAs, which keeps the
// counted vmcnt waits exact.
// Chip-wide pacing (r05): in the full-tile phases every kChipPaceEvery-th XCD pacing
// point also waits for all G blocks on one more counter (same bounded spin), which
// keeps the eight XCDs within ~128 K-tiles (~128 MB of the XP image) of each other,
// so a panel's K-tile fetched from HBM by one XCD is still in the Infinity Cache when
// the other XCDs that use the panel read it.  Interleaved A/B at config 3 (one
// process, bit-identical, profiles/r05zb_syrk_chip_pacing_ab.log): 296.6 -> 283.7 ms
// per op at every 2nd point; every point 286.0, every 3rd 286.5, every 4th 294.0;
// chip-wide only (no XCD level) 292.5; XCD pacing off 327.8.  Remainder rounds with
// global item numbering are chip-paced too, against the round's item count (config 2,
// all remainder: 24.77 -> 24.54 ms; config 3 286.0 -> 284.8).  Config 5 (short K per
// tile) is unchanged.
constexpr int kChipPaceEvery = 2;
// flush stagger per XCD = flush_kt / kFlushStaggerDiv K-tiles (0: none)
#ifdef DEIG_AB_SYRK_FLUSH_STAGGER
constexpr int kFlushStaggerDiv = DEIG_AB_SYRK_FLUSH_STAGGER;
#else
constexpr int kFlushStaggerDiv = 16;
#endif

__device__ __noinline__ void xcd_pace(unsigned* ctr, unsigned target) {
  __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t t0 = wall_clock64();
  while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    if (wall_clock64() - t0 > 2000) break;
    __builtin_amdgcn_s_sleep(1);
  }
}

// Blocks of XCD b & 7 in a grid of G (round-robin dispatch).
__device__ __forceinline__ unsigned xcd_blocks(const SSched& s) {
  const int xcd = blockIdx.x & 7;
  return (unsigned)((s.G >> 3) + (xcd < (s.G & 7) ? 1 : 0));
}

// Pacing points of one work item: every pace_kt K-tiles, n times (n = 0: none); point j
// (1..n) waits for the XCD's counter to reach base + j * mult.
struct PaceSeq {
  int n;
  unsigned base, mult;
  unsigned gbase = 0;  // the chip-wide counter's target before this item
  unsigned gmult = 0;  // blocks that pace chip-wide with this one (G, or a round's items)
  bool g = false;      // every kChipPaceEvery-th point is also chip-wide
};

// Where a block stands in its item's PaceSeq; pace_point is called once per K-tile.
struct PaceState {
  int since = 0, left, gcount = 0;
  unsigned target, gtarget;
  __device__ __forceinline__ explicit PaceState(const PaceSeq& pc)
      : left(pc.n), target(pc.base), gtarget(pc.gbase) {}
};

__device__ __forceinline__ void pace_point(const SSched& s, const PaceSeq& pc, PaceState& p) {
  if (p.left > 0 && ++p.since == s.pace_kt) {
    p.since = 0;
    --p.left;
    p.target += pc.mult;
    if (threadIdx.x == 0) xcd_pace(s.pace + 32 * (blockIdx.x & 7), p.target);
    if (pc.g && ++p.gcount == kChipPaceEvery) {  // ... and every other one chip-wide
      p.gcount = 0;
      p.gtarget += pc.gmult;
      if (threadIdx.x == 0) xcd_pace(s.pace + 32 * 8, p.gtarget);
    }
  }
}

// ---------------------------------------------------------------- work items
// Both persistent kernels run the same schedule.  Full phases (w < q): block L runs all
// K of tile w G + L, in lock-step with the rest.  Remainder: R tiles x nseg equal K
// segments, item i = seg * R + r, taken by logical block i mod G in round i / G; its
// partial sum goes to slab i.  Segment-major numbering keeps the items that run together
// (and, by the XCD-aware relabel, the ~G/8 on one XCD) on the same K rows of neighbouring
// tiles, so their panels are shared in L2 rather than each item streaming its own K range
// from HBM.

// Blocks of this block's XCD (logical L) that run a remainder item in round u: item
// i = L + u G (the XCD's blocks are logical [L - b/8, + nx)).
__device__ __forceinline__ int rem_active(const SSched& s, int L, int u) {
  const int nx = (int)xcd_blocks(s);
  const int left = s.R * s.nseg - u * s.G - (L - (int)(blockIdx.x >> 3));
  return left < 0 ? 0 : (left < nx ? left : nx);
}

__device__ __forceinline__ int rem_rounds(const SSched& s, int L) {
  const int items = s.R * s.nseg;
  return L < items ? (items - 1 - L) / s.G + 1 : 0;
}

// Round u's item of block L: tile index, slot (= segment * R + r) and segment.
__device__ __forceinline__ void rem_item(const SSched& s, int L, int u, int& tile, int& slot, int& sg) {
  const int i = L + u * s.G;
  sg = i / s.R;
  const int r = i - sg * s.R;
  tile = s.q * s.G + r;
  slot = sg * s.R + r;
}

struct WorkItem {
  int tile, slot, seg;  // index into s.order; remainder slab and K segment (0 in full phases)
  int64_t k0, k1;       // K-tiles [k0, k1)
  bool partial;         // a remainder item: the sum goes to slab `slot`, not to S
  PaceSeq pc;
};

// Work item w (< q + rem_rounds) of logical block L, with its pacing sequence.
// Full phases: every block runs P = NK / pace_kt points per tile, so phase w's point j
// (1..P) waits for (w P + j) nx arrivals of the XCD's nx blocks: PaceSeq{P, w P nx, nx}.
// (A running arrival index w P + j times nx, counted through the phases without a bound
// per item, gives the same targets: a full phase's NK K-tiles hold exactly P points.)
// The kernels differ in one thing, HALF (syrks_h_kernel) against the fused syrks_kernel:
// HALF also paces every kChipPaceEvery-th point chip-wide (all G blocks) and paces the
// remainder items - Pm points per item, Pm from the shortest segment, so every item of a
// round runs the same count and the targets stay exact across rounds: XCD-wide against
// the XCD's blocks active in the round, chip-wide against the round's item count.  The
// fused kernel paces its full phases at the XCD level only (remainder: n = 0).
template <bool HALF>
__device__ __forceinline__ WorkItem work_item(const SSched& s, int L, int w) {
  WorkItem it{0, 0, 0, 0, s.NK, w >= s.q, PaceSeq{0, 0u, 0u}};
  const unsigned nx = xcd_blocks(s);
  const unsigned P = s.pace_kt > 0 ? (unsigned)(s.NK / s.pace_kt) : 0u;
  if (!it.partial) {
    it.tile = w * s.G + L;
    it.pc = PaceSeq{(int)P, (unsigned)w * P * nx, nx};
    if (HALF) {
      it.pc.g = true;
      it.pc.gbase = (unsigned)w * (P / kChipPaceEvery) * (unsigned)s.G;
      it.pc.gmult = (unsigned)s.G;
    }
    return it;
  }
  const int u = w - s.q;
  rem_item(s, L, u, it.tile, it.slot, it.seg);
  // (64-bit divisions run on the VALU: pin the bounds to SGPRs, the DMA descriptors
  // built from them must be wave-uniform)
  it.k0 = __builtin_amdgcn_readfirstlane((int)(s.NK * it.seg / s.nseg));
  it.k1 = __builtin_amdgcn_readfirstlane((int)(s.NK * (it.seg + 1) / s.nseg));
  const int Pm = (HALF && s.pace_kt > 0 && s.nseg > 0) ? (int)(s.NK / s.nseg / s.pace_kt) : 0;
  if (Pm > 0) {
    const int items = s.R * s.nseg;
    unsigned before = 0;  // arrivals of the earlier rounds: XCD-wide, chip-wide
    unsigned gb = (unsigned)s.q * (P / kChipPaceEvery) * (unsigned)s.G;
    for (int v = 0; v < u; ++v) {
      before += (unsigned)rem_active(s, L, v);
      gb += (unsigned)min(s.G, items - v * s.G) * (unsigned)(Pm / kChipPaceEvery);
    }
    it.pc = PaceSeq{Pm, (unsigned)s.q * P * nx + before * (unsigned)Pm, (unsigned)rem_active(s, L, u)};
    it.pc.g = true;
    it.pc.gbase = gb;
    it.pc.gmult = (unsigned)min(s.G, items - u * s.G);
  }
  return it;
}

// LDS ring geometry: a K-tile is 32 rows; a panel's K-tile is its 8 (octet, hi|lo)
// slices = 32 KiB, a ring buffer holds the A and the B panel of one K-tile.
constexpr int PANEL_B = 8 * SLICE_B;
constexpr int BUF_B = 2 * PANEL_B;

// ------------------------------------------------ fused split (d <= kFusedMaxD)
// X is staged as it lies in HBM (fp32 rows) and split in LDS, so no XP image is
// written and re-read (the split pass moved 2 x 4nd bytes).  A K-tile is 32 rows;
// wave w owns octet w & 3 of panel w >> 2 (diagonal tiles: panel A twice): it
// DMAs those 8 rows x 256 features (8 x 1 KiB) into the 8 KiB that the octet's
// (hi, lo) slices occupy, and later overwrites them in place with the slices.
// The region is the wave's own, so the split needs no barrier of its own.
constexpr int OCT_B = 2 * SLICE_B;

// One descriptor per stage: base = the octet's first row, records = its rows
// below nrows (later rows read as out of range, and an out-of-range LDS-DMA
// writes zeros); voff = 16 * lane, or an out-of-range offset (2^30 + row offset
// >= every record count, as ldx <= 2^25) for lanes whose features are >= d.
__device__ __forceinline__ void stage_x(const SSched& s, int64_t kt, int f0, unsigned char* buf,
                                        int wave, int voff) {
  const int64_t row0 = kt * 32 + 8 * (wave & 3);
  int64_t rv = s.nrows - row0;
  rv = rv < 0 ? 0 : rv > 8 ? 8 : rv;
  const uint32_t ldx4 = (uint32_t)s.ldx * 4u;
  const i32x4 rsrc = make_rsrc(s.X + row0 * s.ldx + f0, (uint32_t)rv * ldx4);
  unsigned char* dst = buf + (wave >> 2) * PANEL_B + (wave & 3) * OCT_B;
#pragma unroll
  for (int r = 0; r < 8; ++r) dma16(rsrc, voff + (int)(r * ldx4), dst + r * 1024);
}

// Split the wave's staged region in place.  Lane c holds features 2c, 2c + 1 (half
// h = 0) and 128 + 2c, 129 + 2c (h = 1) of the 8 rows; all 16 reads land before
// the first write (the slices overlap every staged row).  Rows >= nrows and
// features >= d are zeroed here (independent of what a dropped DMA left in LDS).
// SQ: also accumulate the dropped lo * lo diagonal term (as r^2, r = x - hi: the
// difference is ~2^-25 x^2) into sq[2h + e].
template <bool SQ>
__device__ __forceinline__ void convert_x(unsigned char* buf, int wave, int lane, int rv, int fv,
                                          float* sq) {
  unsigned char* R = buf + (wave >> 2) * PANEL_B + (wave & 3) * OCT_B;
  f32x2 v[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 8; ++r)
      v[h][r] = *reinterpret_cast<const f32x2*>(R + r * 1024 + h * 512 + 8 * lane);
  if (rv < 8 || fv < 256) {  // wave-uniform: the ragged last K-tile / a panel past d
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (r >= rv || 128 * h + 2 * lane >= fv) v[h][r] = f32x2{0.f, 0.f};
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      u32x4 hv, lv;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float x0 = v[h][2 * p][e], x1 = v[h][2 * p + 1][e];
        const uint32_t hh = cvt2(x0, x1);
        const float r0 = x0 - lo_f(hh), r1 = x1 - hi_f(hh);
        hv[p] = hh;
        lv[p] = cvt2(r0, r1);
        if (SQ) sq[2 * h + e] = fmaf(r0, r0, fmaf(r1, r1, sq[2 * h + e]));
      }
      const int f = 128 * h + 2 * lane + e;
      *reinterpret_cast<u32x4*>(R + f * 16) = hv;
      *reinterpret_cast<u32x4*>(R + SLICE_B + f * 16) = lv;
    }
}

// ---------------------------------------------------------------- accumulators
// A wave's 128 x 64 output tile in the result registers of v_mfma_f32_16x16x32_bf16:
// 8 x 4 blocks of f32x4, viewed as 32 "quads" - 4 consecutive rows ib..ib+3 of one
// column j - which is how they are flushed, spilled to slabs and stored.
struct Acc {
  f32x4 a[8][4];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int mb = 0; mb < 8; ++mb)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) a[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // quad q = (mb, nb): rows 16 mb + 4 (lane / 16), column 16 nb + lane % 16
  __device__ __forceinline__ float at(int q, int u) const { return a[q >> 2][q & 3][u]; }
  __device__ __forceinline__ void set(int q, int u, float v) { a[q >> 2][q & 3][u] = v; }
  static __device__ __forceinline__ int qrow(int q, int lane) { return 16 * (q >> 2) + 4 * (lane >> 4); }
  static __device__ __forceinline__ int qcol(int q, int lane) { return 16 * (q & 3) + (lane & 15); }

  // One K-tile (32 rows) = one 32-deep MFMA step; operand slice of 8 k-values:
  // octet lane / 16 (conflict-free ds_read_b128 lane groups).
  __device__ __forceinline__ void mma(const unsigned char* A, const unsigned char* B, int wi,
                                      int wj, int lane) {
    const int c = lane & 15, o = lane >> 4;
    {
      const unsigned char* ph = A + ((o * 2) * BT + 128 * wi + c) * 16;
      const unsigned char* qh = B + ((o * 2) * BT + 64 * wj + c) * 16;
      bf16x8 bhi[4], blo[4];
      // A block mb + 1 is read while block mb's 12 MFMAs run (two A register
      // sets), so only the first read of a k-step exposes LDS latency.
      bf16x8 ahi = *reinterpret_cast<const bf16x8*>(ph);
      bf16x8 alo = *reinterpret_cast<const bf16x8*>(ph + BT * 16);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        bhi[nb] = *reinterpret_cast<const bf16x8*>(qh + (16 * nb) * 16);
        blo[nb] = *reinterpret_cast<const bf16x8*>(qh + (BT + 16 * nb) * 16);
      }
#pragma unroll
      for (int mb = 0; mb < 8; ++mb) {
        bf16x8 nhi = ahi, nlo = alo;
        if (mb + 1 < 8) {
          nhi = *reinterpret_cast<const bf16x8*>(ph + (16 * (mb + 1)) * 16);
          nlo = *reinterpret_cast<const bf16x8*>(ph + (BT + 16 * (mb + 1)) * 16);
        }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          a[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bhi[nb], a[mb][nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          a[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, blo[nb], a[mb][nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          a[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bhi[nb], a[mb][nb], 0, 0, 0);
        ahi = nhi;
        alo = nlo;
      }
      // Issue order for the scheduler: A0 + B reads, then per block the next
      // block's two A reads ahead of the current block's 12 MFMAs.
      __builtin_amdgcn_sched_group_barrier(0x100, 10, 0);
#pragma unroll
      for (int mb = 0; mb < 8; ++mb) {
        if (mb + 1 < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
      }
    }
  }
};

constexpr int NQUAD = 32;

// Slab image: quad-major, 16 B per lane (the reduce kernel reads it back).
__device__ __forceinline__ f32x4* slab_at(float* slab, int wave, int q, int lane) {
  return reinterpret_cast<f32x4*>(slab + ((wave * NQUAD + q) * 64 + lane) * 4);
}

// The slab addresses are formed here from an opaque base: otherwise the compiler
// hoists all 32 of them out of the K loop and keeps 64 VGPRs live for them.
// r06: buffer loads / stores in batches of kFlushBatch quads.  Through a generic
// pointer the slab accesses were flat_* operations, which the hardware may complete
// out of order, so each quad's read was its own vmcnt(0) round trip: 32 serial round
// trips per flush (~34 us per event at config 3).  Buffer operations complete in issue
// order, so a batch's reads are in flight together (its write-backs stay queued
// behind them).
#ifdef DEIG_AB_SYRK_FLUSH_BATCH
constexpr int kFlushBatch = DEIG_AB_SYRK_FLUSH_BATCH;
#else
constexpr int kFlushBatch = 4;
#endif
__device__ __forceinline__ void flush(float* slab, bool first, Acc& acc, int wave, int lane) {
  asm volatile("" : "+v"(slab));
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(slab, (short)0, (int)(SLAB * sizeof(float)), 0x00020000);
  const int voff = (wave * NQUAD * 64 + lane) * 16;
  auto put = [&](int q, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff + q * 1024, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc.set(q, u, 0.f);
  };
  if (first) {
#pragma unroll
    for (int q = 0; q < NQUAD; ++q) put(q, f32x4{acc.at(q, 0), acc.at(q, 1), acc.at(q, 2), acc.at(q, 3)});
    return;
  }
#pragma unroll
  for (int b = 0; b < NQUAD; b += kFlushBatch) {
    f32x4 v[kFlushBatch];
#pragma unroll
    for (int i = 0; i < kFlushBatch; ++i)
      v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + (b + i) * 1024, 0, 0));
    __builtin_amdgcn_sched_barrier(0);  // the batch's reads issue together
#pragma unroll
    for (int i = 0; i < kFlushBatch; ++i) {
      const int q = b + i;
      put(q, v[i] + f32x4{acc.at(q, 0), acc.at(q, 1), acc.at(q, 2), acc.at(q, 3)});
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

__device__ __forceinline__ void unflush(float* slab, Acc& acc, int wave, int lane) {
  asm volatile("" : "+v"(slab));
  // buffer loads in batches (flat loads were one vmcnt(0) round trip each, see flush)
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(slab, (short)0, (int)(SLAB * sizeof(float)), 0x00020000);
  const int voff = (wave * NQUAD * 64 + lane) * 16;
#pragma unroll
  for (int b = 0; b < NQUAD; b += kFlushBatch) {
    f32x4 v[kFlushBatch];
#pragma unroll
    for (int i = 0; i < kFlushBatch; ++i)
      v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + (b + i) * 1024, 0, 0));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kFlushBatch; ++i)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc.set(b + i, u, acc.at(b + i, u) + v[i][u]);
  }
}

// Store 4 consecutive rows ib..ib+3 of column j (values = alpha * a[u] (+ S)),
// into S[i][j] and the mirror S[j][i].  Diagonal tiles keep only i >= j, so both
// triangles come from the same register (bit-exact symmetry).
__device__ __forceinline__ void store4(const SSched& s, int ib, int j, bool diag, const float* a) {
  if (ib >= s.d || j >= s.d) return;
  float v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float* p = s.S + (int64_t)(ib + u) * s.lds + j;
    v[u] = s.alpha * a[u];
    if (s.beta && (!diag || ib + u >= j)) v[u] += *p;
  }
  if (!diag) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s.S[(int64_t)(ib + u) * s.lds + j] = v[u];
    const f32x4 w = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(s.S + (int64_t)j * s.lds + ib) = w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ib + u >= j) {
        s.S[(int64_t)(ib + u) * s.lds + j] = v[u];
        s.S[(int64_t)j * s.lds + ib + u] = v[u];
      }
  }
}

// A wave's place in its block's tile, and the slab the block flushes into (full phases:
// the block's own) or leaves its partial sum in (remainder items: the item's).
struct TileCtx {
  int lane, wave, wi, wj;  // wave tile: rows 128 wi, columns 64 wj of the tile
  int ti, tj, i0, j0;      // tile coordinates, in tiles and in features
  bool diag;
  float* slab;
};

__device__ __forceinline__ TileCtx tile_ctx(const SSched& s, const WorkItem& it) {
  TileCtx c;
  c.lane = threadIdx.x & 63;
  c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  c.wi = c.wave >> 2;
  c.wj = c.wave & 3;
  const int tt = __builtin_amdgcn_readfirstlane(s.order[it.tile]);
  c.ti = tt & 0xffff;
  c.tj = tt >> 16;
  c.i0 = c.ti * BT;
  c.j0 = c.tj * BT;
  c.diag = (c.ti == c.tj);
  c.slab = it.partial ? s.part + (int64_t)it.slot * SLAB : s.accs + (int64_t)blockIdx.x * SLAB;
  return c;
}

// After the K loop: add back what was flushed, then leave the wave's 32 quads in the
// item's slab (remainder) or store them to S.  IDLE: a wave whose block lies wholly above
// the diagonal holds zeros - it never flushed and stores nothing to S, but still writes
// its part of a partial slab (the reduce kernel reads the whole slab).
// The context comes by value: through a reference the stores to S might alias it, and
// every store4 then forms its addresses anew with full 64-bit multiplies.
template <bool IDLE = false>
__device__ __forceinline__ void finish_tile(const SSched& s, const TileCtx c, Acc& acc, bool flushed,
                                            bool partial) {
  if constexpr (!IDLE)
    if (flushed) unflush(c.slab, acc, c.wave, c.lane);
  if (partial) {
#pragma unroll
    for (int q = 0; q < NQUAD; ++q)
      *slab_at(c.slab, c.wave, q, c.lane) = f32x4{acc.at(q, 0), acc.at(q, 1), acc.at(q, 2), acc.at(q, 3)};
    return;
  }
  if constexpr (IDLE) return;
#pragma unroll
  for (int q = 0; q < NQUAD; ++q) {
    const float a[4] = {acc.at(q, 0), acc.at(q, 1), acc.at(q, 2), acc.at(q, 3)};
    store4(s, c.i0 + 128 * c.wi + Acc::qrow(q, c.lane), c.j0 + 64 * c.wj + Acc::qcol(q, c.lane), c.diag, a);
  }
}

// One work item of the fused kernel: K-tiles [k0, k1) of a tile on a two-stage ring.
template <bool SQ>
__device__ __forceinline__ void segment(const SSched& s, unsigned char* lds, const WorkItem& it) {
  const TileCtx tc = tile_ctx(s, it);
  const int lane = tc.lane, wave = tc.wave, wi = tc.wi, wj = tc.wj;
  const int64_t k0 = it.k0;
  float* const slab = tc.slab;
  // fused split: this wave's panel origin, valid features in it, DMA lane offset
  const int fx0 = (wave >= 4 && !tc.diag) ? tc.j0 : tc.i0;
  const int fv = s.d - fx0;
  const int xvoff = 4 * lane < fv ? lane * 16 : (1 << 30);
  // lo^2 of the diagonal: panel A's octets (waves 0-3) of diagonal tiles
  float sq[4] = {0.f, 0.f, 0.f, 0.f};

  Acc acc;
  acc.zero();
  bool flushed = false;
  const int64_t nkt = it.k1 - k0;
  if (nkt > 0) {
    // Nothing else may be in flight on the VM counter while the ring runs (the
    // counted waits assume only DMAs): drain the previous segment's stores.
    wait_vm<0>();
    __syncthreads();  // the previous segment's last stage may still be read
    // Ring of two stages: stage t lives in buffer t % 2.  K-tile k0 is staged and
    // split (masked: it may be ragged) before the loop; iteration t stages K-tile
    // t + 1 after the barrier and splits it inside K-tile t's MFMAs (its own region:
    // a vmcnt wait, no barrier).
    stage_x(s, k0, fx0, lds, wave, xvoff);
    wait_vm<0>();
    const int64_t rv0 = s.nrows - (k0 * 32 + 8 * (wave & 3));
    convert_x<SQ>(lds, wave, lane, rv0 < 0 ? 0 : rv0 > 8 ? 8 : (int)rv0, fv, sq);
    int cur = 0, nxt = 1, since = 0;
    PaceState pace(it.pc);
    for (int64_t t = 0; t < nkt; ++t) {
      pace_point(s, it.pc, pace);
      // RAW: every wave split its own region of stage t last iteration (its
      // ds_writes retire at the lgkmcnt wait), so the barrier publishes stage t.
      // WAR: stage t-1's ds_reads retired (lgkmcnt) before the barrier, so its
      // buffer can be restaged right after it.  A raw s_barrier: __syncthreads()
      // would also wait for vmcnt(0).
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (t + 1 < nkt) stage_x(s, k0 + t + 1, fx0, lds + nxt * BUF_B, wave, xvoff);
      // K-tile t's MFMAs, then this wave's split of K-tile t + 1 (its DMAs were
      // issued right after the barrier: the MFMAs cover their latency).  The
      // in-place split of the wave's own region needs no barrier of its own.
      unsigned char* bc = lds + cur * BUF_B;
      acc.mma(bc, bc + PANEL_B, wi, wj, lane);
      if (t + 1 < nkt) {
        wait_vm<0>();
        const int64_t rv1 = s.nrows - ((k0 + t + 1) * 32 + 8 * (wave & 3));
        convert_x<SQ>(lds + nxt * BUF_B, wave, lane, rv1 < 0 ? 0 : rv1 > 8 ? 8 : (int)rv1, fv, sq);
      }
      if (++since == s.flush_kt && t + 1 < nkt) {
        flush(slab, !flushed, acc, wave, lane);
        wait_vm<0>();  // keep the slab traffic off the ring's counted waits
        flushed = true;
        since = 0;
      }
      cur = cur + 1 == 2 ? 0 : cur + 1;
      nxt = nxt + 1 == 2 ? 0 : nxt + 1;
    }
  }
  if (SQ) {  // [segment][octet wave][dp]; summed by diag_corr_kernel
    float* c = s.corr + (int64_t)(it.seg * 4 + wave) * s.dp + tc.i0;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      *reinterpret_cast<f32x2*>(c + 128 * h + 2 * lane) = f32x2{sq[2 * h], sq[2 * h + 1]};
  }
  finish_tile(s, tc, acc, flushed, it.partial);
}

// ------------------------------------------------ half-refill ring (d > kFusedMaxD)
// Two phases per K-tile (48-MFMA M parts), waves 4-7 one barrier behind waves 0-3: a
// ring buffer is four A quarters (8 KiB: features 32 q .. 32 q + 31 and 128 + the same
// of all 8 slices) and the B panel; phase h reads A quarters 2h and
// 2h + 1 (and B in phase 0), and each region is restaged with K-tile t + 2 as soon as
// both wave groups have read it.  Per wave and K-tile 8 pieces in two L parts of 4:
//   L_0(t): B(t+1) parts 2, 3 and A quarters 2, 3 of t+1 into nxt (their previous
//           contents, K-tile t-1's B and second half, were read by both groups by
//           the barrier that opened this part);
//   L_1(t): B(t+2) parts 0, 1 and A quarters 0, 1 of t+2 into cur (read in L_0(t)).
// So every piece has ~1.5 K-tiles of lead instead of one.  RAW: a wave waits for its
// own pieces of a region at the end of the L part before the one that reads it:
// end of L_0(t) for A quarters 2, 3 of t (younger: L_1(t-1)'s 4 + L_0(t)'s 4 = 8);
// end of L_1(t) for K-tile t+1's B and quarters 0, 1 (younger than its last piece,
// B part 3 issued in L_0(t): quarters 2, 3 of t+1 + L_1(t)'s 4 = 6).  Near the end of
// the segment the counts shrink with the pieces not issued.  WAR: every L part
// retires its reads (lgkmcnt(0)) before its closing barrier.  Same MFMA order per
// accumulator as the fused kernel (Acc::mma).
// DW != -1: a DIAGONAL tile.  Its B panel is its A panel, so no B pieces are staged
// and the B operands are read from the A quarters (the same bytes in the A layout);
// with 2 DMA pieces per L part instead of 4 the counted waits become 4 / 2, and the end
// of L_1 also waits for quarters 2, 3 of the next K-tile (phase 0 reads them as B).
// The same B-operand read point and restage points as before, so the WAR argument
// above holds unchanged.
// DW >= 0: a wave of a diagonal tile whose 128 x 64 block starts DW = 64 wj - 128 wi
// columns right of the diagonal (0, 64, or 128 for waves 2 and 3 alike, whose blocks lie
// wholly above it; waves 4 and 5 of the tile run DW = -2).
// store4 keeps only i >= j there, so the 16 x 16 MFMA blocks that lie wholly above the
// diagonal (dw_skip) are neither computed nor their operands read: all of waves 2 and
// 3 (DW = 128: they only stage their DMA pieces and pass the barriers), 22 of 32 blocks
// of waves 1 and 7, 6 of waves 0 and 6 - 120 of the tile's 256, MFMAs a power-held
// chip does not spend.  Every stored sum is the same MFMA chain as before
// (bit-identical); separate instantiations, so the other tiles' code is unchanged (a
// runtime test inside the loop measured slower, r06).
constexpr int kDwOff = -1, kDwDiag = -2;
constexpr bool dw_skip(int dw, int mb, int nb) { return dw >= 0 && 16 * mb + 15 < dw + 16 * nb; }
constexpr bool dw_row(int dw, int mb) { return !dw_skip(dw, mb, 0); }  // A block row mb is read
constexpr bool dw_col(int dw, int nb) { return !dw_skip(dw, 7, nb); }  // B block column nb is read
constexpr bool dw_idle(int dw) { return !dw_row(dw, 7); }

template <int DW>
__device__ __forceinline__ void segment_h(const SSched& s, unsigned char* lds, const WorkItem& it) {
  constexpr bool idle = dw_idle(DW);
  constexpr bool dgb = DW != kDwOff;  // B operands from the A quarters
  constexpr int QB = 8 * 1024;  // one A quarter
  constexpr int BOFF = 4 * QB;  // the B panel
  const TileCtx tc = tile_ctx(s, it);
  const int lane = tc.lane, wave = tc.wave, wi = tc.wi, wj = tc.wj, ti = tc.ti, tj = tc.tj;
  const bool lag = wave >= 4;
  const int64_t k0 = it.k0;
  float* const slab = tc.slab;
  Acc acc;
  acc.zero();
  bool flushed = false;
  const int64_t nkt = it.k1 - k0;
  auto bar = [&]() {  // raw barrier; nothing moves across it
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
  };
  const int a_off = ti * BLOCK_B + wave * SLICE_B + ((lane >> 5) * 128 + (lane & 31)) * 16;
  const int b_off = tj * BLOCK_B + wave * SLICE_B + lane * 16;
  const uint32_t nrec = (uint32_t)(s.nt * BLOCK_B);
  auto ring_rsrc = [&](int64_t kt) {
    return make_rsrc(s.XP + kt * (int64_t)s.nt * BLOCK_B, nrec);
  };
  auto issue_a = [&](int64_t kt, int q, unsigned char* buf) {
    const i32x4 r = ring_rsrc(kt);
    int o = a_off + q * 512;
    asm volatile("" : "+v"(o));
    dma16(r, o, buf + q * QB + wave * 1024);
  };
  auto issue_b = [&](int64_t kt, unsigned char* buf, int p0, int p1) {
    const i32x4 r = ring_rsrc(kt);
    int o = b_off;
    asm volatile("" : "+v"(o));
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p >= p0 && p < p1) dma16(r, o + p * 1024, buf + BOFF + wave * SLICE_B + p * 1024);
  };
  if (nkt > 0) {
    wait_vm<0>();     // the previous segment's stores / flushes
    __syncthreads();  // ... and its last reads of the ring
    // K-tile k0 whole, then K-tile k0 + 1's B parts 0, 1 and quarters 0, 1 (as an
    // L_1 of K-tile k0 - 1 would have issued them)
    if constexpr (!dgb) issue_b(k0, lds, 0, 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) issue_a(k0, q, lds);
    if (nkt > 1) {
      if constexpr (!dgb) issue_b(k0 + 1, lds + BUF_B, 0, 2);
      issue_a(k0 + 1, 0, lds + BUF_B);
      issue_a(k0 + 1, 1, lds + BUF_B);
      wait_vm<dgb ? 2 : 4>();  // K-tile k0 landed
    } else {
      wait_vm<0>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bar();
    if (lag) bar();  // the stagger
    const int c = lane & 15, g4 = lane >> 4;
    const int xcd = blockIdx.x & 7;
    // Flush stagger (r06): XCD x flushes x * flush_kt / 16 K-tiles earlier than XCD 0,
    // so the eight XCDs' slab bursts fall at different K-tiles instead of all at once
    // (each partial sum still spans flush_kt K-tiles, the first one of a segment fewer).
    int since = kFlushStaggerDiv > 0 ? xcd * (s.flush_kt / kFlushStaggerDiv) : 0;
    PaceState pace(it.pc);
    bf16x8 bhi[4], blo[4];
    bf16x8 ahi[4], alo[4];
    for (int64_t t = 0; t < nkt; ++t) {
      unsigned char* cur = lds + (t & 1) * BUF_B;
      unsigned char* nxt = lds + ((t + 1) & 1) * BUF_B;
      const bool has1 = t + 1 < nkt, has2 = t + 2 < nkt;
      const unsigned char* pa = cur + ((g4 * 2) * 64 + 32 * wi + c) * 16;
      const unsigned char* pb = cur + BOFF + ((g4 * 2) * BT + 64 * wj + c) * 16;
      // B feature f = 64 wj + 16 nb + c of slice 2 g4 (+1: lo) in the A layout:
      // quarter (f % 128) / 32, lane 32 (f / 128) + f % 32
      const unsigned char* pbd = cur + (2 * (wj & 1)) * QB + (2 * g4) * 1024 + (32 * (wj >> 1) + c) * 16;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // ---------------- L part
        if (h == 0) {
          pace_point(s, it.pc, pace);
          if (since == s.flush_kt) {
            if constexpr (!idle) flush(slab, !flushed, acc, wave, lane);
            wait_vm<0>();
            flushed = true;
            since = 0;
          }
          ++since;
          if (has1) {
            if constexpr (!dgb) issue_b(k0 + t + 1, nxt, 2, 4);
            issue_a(k0 + t + 1, 2, nxt);
            issue_a(k0 + t + 1, 3, nxt);
          }
#pragma unroll
          for (int nb = 0; nb < 4; ++nb) {
            if (dw_col(DW, nb)) {
              if constexpr (dgb) {
                const unsigned char* pq = pbd + (nb >> 1) * QB + (16 * (nb & 1)) * 16;
                bhi[nb] = *reinterpret_cast<const bf16x8*>(pq);
                blo[nb] = *reinterpret_cast<const bf16x8*>(pq + 1024);
              } else {
                bhi[nb] = *reinterpret_cast<const bf16x8*>(pb + (16 * nb) * 16);
                blo[nb] = *reinterpret_cast<const bf16x8*>(pb + (BT + 16 * nb) * 16);
              }
            }
          }
        } else if (has2) {
          if constexpr (!dgb) issue_b(k0 + t + 2, cur, 0, 2);
          issue_a(k0 + t + 2, 0, cur);
          issue_a(k0 + t + 2, 1, cur);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int q = 2 * h + (m >> 1), mm = m & 1;
          if (dw_row(DW, 4 * h + m)) {
            ahi[m] = *reinterpret_cast<const bf16x8*>(pa + q * QB + (16 * mm) * 16);
            alo[m] = *reinterpret_cast<const bf16x8*>(pa + q * QB + (64 + 16 * mm) * 16);
          }
        }
        if constexpr (dgb) {  // 2 pieces per L part; phase 0 reads all four quarters
          if (h == 0) {
            if (has1) wait_vm<4>(); else wait_vm<0>();
          } else {
            if (has2) wait_vm<2>(); else wait_vm<0>();
          }
        } else if (h == 0) {
          if (has1) wait_vm<8>(); else wait_vm<0>();
        } else {
          if (has2) wait_vm<6>(); else if (has1) wait_vm<2>(); else wait_vm<0>();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bar();
        // ---------------- M part
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int mb = 4 * h + m;
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
            if (!dw_skip(DW, mb, nb))
              acc.a[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[m], bhi[nb], acc.a[mb][nb], 0, 0, 0);
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
            if (!dw_skip(DW, mb, nb))
              acc.a[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[m], blo[nb], acc.a[mb][nb], 0, 0, 0);
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
            if (!dw_skip(DW, mb, nb))
              acc.a[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo[m], bhi[nb], acc.a[mb][nb], 0, 0, 0);
        }
        bar();
      }
    }
    if (!lag) bar();  // balance the stagger
  }
  finish_tile<idle>(s, tc, acc, flushed, it.partial);
}

__global__ __launch_bounds__(NTHR) void syrks_h_kernel(SSched s) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_B];
  const int L = xcd_logical(blockIdx.x, s.G);
  const int nwork = s.q + rem_rounds(s, L);
  for (int w = 0; w < nwork; ++w) {
    const WorkItem it = work_item<true>(s, L, w);
    const int tt = __builtin_amdgcn_readfirstlane(s.order[it.tile]);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool dg = (tt & 0xffff) == (tt >> 16);
    const int dw = 64 * (wv & 3) - 128 * (wv >> 2);
    if (dg && dw == 0)
      segment_h<0>(s, lds, it);
    else if (dg && dw == 64)
      segment_h<64>(s, lds, it);
    else if (dg && dw >= 128)  // waves 2 and 3: the whole block above the diagonal
      segment_h<128>(s, lds, it);
    else if (dg)
      segment_h<kDwDiag>(s, lds, it);
    else
      segment_h<kDwOff>(s, lds, it);
  }
}

// The fused-split kernel (d <= kFusedMaxD): persistent, one block per CU.
__global__ __launch_bounds__(NTHR) void syrks_kernel(SSched s) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_B];
  const int L = xcd_logical(blockIdx.x, s.G);
  const int nwork = s.q + rem_rounds(s, L);
  for (int w = 0; w < nwork; ++w) {
    const WorkItem it = work_item<false>(s, L, w);
    // the lo^2 accumulation is compiled only into the copy that the diagonal tiles'
    // A-panel waves run
    const int tt = __builtin_amdgcn_readfirstlane(s.order[it.tile]);
    if ((tt & 0xffff) == (tt >> 16) && (threadIdx.x >> 6) < 4)
      segment<true>(s, lds, it);
    else
      segment<false>(s, lds, it);
  }
}

// grid (R, SLAB/4/256): one thread per float4 of a remainder tile's slab image.
__global__ __launch_bounds__(256) void syrks_reduce_kernel(SSched s) {
  const int r = blockIdx.x;
  const int f = blockIdx.y * 256 + threadIdx.x;
  const int lane = f & 63, q = (f >> 6) & (NQUAD - 1), wave = f >> 11;
  const int wi = wave >> 2, wj = wave & 3;
  const int tt = s.order[s.q * s.G + r];
  const int ti = tt & 0xffff, tj = tt >> 16;
  const bool diag = (ti == tj);
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  for (int sg = 0; sg < s.nseg; ++sg)  // fixed order: deterministic
    sum += *reinterpret_cast<const f32x4*>(s.part + (int64_t)(sg * s.R + r) * SLAB + (int64_t)f * 4);
  const float a[4] = {sum[0], sum[1], sum[2], sum[3]};
  store4(s, ti * BT + 128 * wi + Acc::qrow(q, lane), tj * BT + 64 * wj + Acc::qcol(q, lane),
         diag, a);
}

__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// (r04, measured and not kept: one 16-B load per lane and row, lane -> features
// 4 lane + j, so each hi / lo store covers 16 B at a 64-B stride: config 2 op 27.54 vs
// 25.74 ms, config-3 shard 315.3 vs 307.7, profiles/r04zb_syrk_*_ab.log - most likely
// the stores: below, each wave store instruction writes 1 KiB contiguous.)
// X rows [0, n) of the chunk -> XP (noct octets; rows >= n and features >= d
// are zeros) + per-block partial sums of lo^2 per feature (corr[blockIdx.y][f]).
// grid (dp / 256, YB), 256 threads; lane handles features fb + lane + 64 q.
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ X, int64_t n,
                                                    int64_t ldx, int d, int64_t dp, int64_t noct,
                                                    unsigned char* __restrict__ XP,
                                                    float* __restrict__ corr) {
  __shared__ float red[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t fb = (int64_t)blockIdx.x * 256;
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t o = (int64_t)blockIdx.y * 4 + w; o < noct; o += (int64_t)gridDim.y * 4) {
    float v[4][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int64_t row = o * 8 + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t f = fb + lane + 64 * q;
        v[q][r] = (row < n && f < d) ? __builtin_nontemporal_load(X + row * ldx + f) : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4 hv, lv;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t h0 = bf16_rne(v[q][2 * p]), h1 = bf16_rne(v[q][2 * p + 1]);
        const float r0 = v[q][2 * p] - __uint_as_float(h0 << 16);
        const float r1 = v[q][2 * p + 1] - __uint_as_float(h1 << 16);
        const uint32_t l0 = bf16_rne(r0), l1 = bf16_rne(r1);
        const float lf0 = __uint_as_float(l0 << 16), lf1 = __uint_as_float(l1 << 16);
        sq[q] += lf0 * lf0 + lf1 * lf1;
        hv[p] = h0 | (h1 << 16);
        lv[p] = l0 | (l1 << 16);
      }
      const int64_t f = fb + lane + 64 * q;
      // [32-row block o/4][panel f/256][slice (o%4)*2 + hi|lo][f%256][16 B]
      unsigned char* dst = XP + ((o >> 2) * (dp / BT) + (f / BT)) * BLOCK_B +
                           ((o & 3) * 2) * SLICE_B + (f % BT) * 16;
      // non-temporal: the image is streamed back from HBM by the SYRK anyway (r04,
      // profiles/r04zv_split_nt_stores_ab.log: config-3 shard 298.7 -> 297.8 ms per op,
      // config 2 26.49 -> 26.33, bit-identical)
      __builtin_nontemporal_store(hv, reinterpret_cast<u32x4*>(dst));
      __builtin_nontemporal_store(lv, reinterpret_cast<u32x4*>(dst + SLICE_B));
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[w][lane + 64 * q] = sq[q];
  __syncthreads();
  const int t = threadIdx.x;
  corr[(int64_t)blockIdx.y * dp + fb + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

// S[i][i] += alpha * sum_y corr[y][i]  (the dropped lo * lo term on the diagonal).
// grid (d / 64): 64 features x 4 row slices per block, the slices summed in order
// (r04: one thread per feature over all yb rows took 110 us at config 3 - 32 blocks,
// each thread a 256-long dependent chain of loads; profiles/r04fin_c3_kernel_stats.csv)
__global__ __launch_bounds__(256) void diag_corr_kernel(const float* __restrict__ corr, int yb,
                                                        int64_t dp, int d, float alpha, float* S,
                                                        int64_t lds) {
  __shared__ float part[4][64];
  const int t = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + t;
  float c = 0.f;
  if (i < d) {
#pragma unroll 8
    for (int y = sl; y < yb; y += 4) c += corr[(int64_t)y * dp + i];
  }
  part[sl][t] = c;
  __syncthreads();
  if (sl == 0 && i < d) S[(int64_t)i * lds + i] += alpha * (((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]);
}

// Lower-triangle tiles in super-tile order (SUPER_H tile rows x SUPER_W tile cols).
// One thread per super-tile (r04: one thread for all took 110 us at d = 16384, 8 per
// config-5 step): a super-row starts after the R0 (R0 + 1) / 2 tiles of the rows above,
// a super-tile after its super-row's tiles left of it.
__global__ __launch_bounds__(256) void tile_order_kernel(int nt, int* order) {
  const int nsc = (nt + SUPER_W - 1) / SUPER_W;
  const int u = blockIdx.x * 256 + threadIdx.x;
  const int R0 = (u / nsc) * SUPER_H, C0 = (u % nsc) * SUPER_W;
  if (R0 >= nt) return;
  const int rmax = R0 + SUPER_H < nt ? R0 + SUPER_H : nt;
  if (C0 >= rmax) return;
  int idx = R0 * (R0 + 1) / 2;
  for (int c = 0; c < C0; c += SUPER_W)
    for (int ti = R0; ti < rmax; ++ti) {
      const int hi = c + SUPER_W < ti + 1 ? c + SUPER_W : ti + 1;
      idx += hi > c ? hi - c : 0;
    }
  for (int ti = R0; ti < rmax; ++ti)
    for (int tj = C0; tj < C0 + SUPER_W && tj <= ti; ++tj) order[idx++] = ti | (tj << 16);
}

// K segments per remainder tile: the smallest nseg (<= 64) whose critical path
// ceil(R nseg / G) / nseg (in full-tile passes) is within 2 % of the best.
int remainder_segments(int64_t R, int G) {
  if (R <= 0) return 0;
  double best = 1e30;
  for (int k = 1; k <= 64; ++k) best = fmin(best, (double)cdiv(R * k, G) / k);
  for (int k = 1; k <= 64; ++k)
    if ((double)cdiv(R * k, G) / k <= best * 1.02) return k;
  return 1;
}

// Compact XCD groups (r05; G = 256 blocks, nt % 8 == 0): the triangle of nt / 8 = m
// block rows of 8 tile rows is cut into m diagonal triangles (36 tiles: a group of 32
// on 8 panels plus 4 left over) and m (m - 1) / 2 off-diagonal 8 x 8 squares (two
// groups of 8 x 4 tiles on 12 panels each).  Group g holds order[32 g .. 32 g + 31]; in
// full phase w XCD x runs group 8 w + x (its G / 8 = 32 blocks, one tile each), so an
// XCD's concurrent tiles share 8-12 panels (the 8 x 4 super-tile order averaged 14.5
// at config 3: its 32-tile runs straddle super-tiles); the two halves of a square run in
// the same phase on neighbouring XCDs.  The 4 m leftover tiles end the order: they are
// the split-K remainder (T mod 256 = 4 m whenever m % 4 == 0).  Groups are listed by
// block row a: the triangle, then squares (a, 0 .. a - 1); block row a starts at group
// a^2.  One thread per group.
__global__ __launch_bounds__(256) void tile_order_compact_kernel(int nt, int* order) {
  const int m = nt / 8;
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= m * m) return;
  int a = (int)sqrtf((float)u);
  while (a * a > u) --a;
  while ((a + 1) * (a + 1) <= u) ++a;
  const int item = u - a * a;
  int* grp = order + 32 * u;
  if (item == 0) {
    int i = 0;
    for (int ti = 8 * a; ti < 8 * a + 8; ++ti)
      for (int tj = 8 * a; tj <= ti; ++tj) {
        const int v = ti | (tj << 16);
        if (i < 32) grp[i] = v;
        else order[32 * m * m + 4 * a + (i - 32)] = v;
        ++i;
      }
  } else {
    const int b = (item - 1) >> 1, h = (item - 1) & 1;
    int i = 0;
    for (int ti = 8 * a; ti < 8 * a + 8; ++ti)
      for (int tj = 8 * b + 4 * h; tj < 8 * b + 4 * h + 4; ++tj) grp[i++] = ti | (tj << 16);
  }
}

struct Layout {
  int64_t dp, nt, T, G, q, R, nseg, yb_max, chunk_rows;
  size_t off_order, off_pace, off_accs, off_part, off_corr, off_xp, total;
};

// Workspace: [order][G flush slabs][R * nseg remainder slabs][corr YB x dp][XP chunk].
Layout make_layout(int64_t d, int G, int64_t chunk_rows) {
  Layout L;
  L.dp = cdiv(d, BT) * BT;
  L.nt = L.dp / BT;
  L.T = L.nt * (L.nt + 1) / 2;
  L.G = G;
  L.q = L.T / G;
  L.R = L.T % G;
  L.nseg = remainder_segments(L.R, G);
  L.yb_max = SPLIT_YB;
  L.chunk_rows = chunk_rows;
  size_t off = 0;
  L.off_order = off;
  off = align_up(off + sizeof(int) * L.T, 256);
  L.off_pace = off;
  off += 16 * 128;  // 8 XCD counters and the chip-wide one, one per 128-B line
  L.off_accs = off;
  off += sizeof(float) * (size_t)G * SLAB;
  L.off_part = off;
  off += sizeof(float) * (size_t)(L.R * L.nseg) * SLAB;
  L.off_corr = off;
  off = align_up(off + sizeof(float) * (size_t)L.yb_max * L.dp, 256);
  L.off_xp = off;
  off += (size_t)chunk_rows * L.dp * 4;
  L.total = off;
  return L;
}

int64_t default_chunk_rows(int64_t n, int64_t d) {
  const int64_t dp = cdiv(d, BT) * BT;
  const int64_t n32 = cdiv(n, ROWS_PAD) * ROWS_PAD;
  int64_t cap = (int64_t)(DEFAULT_CHUNK_BYTES / (size_t)(dp * 4)) / ROWS_PAD * ROWS_PAD;
  if (cap < ROWS_PAD) cap = ROWS_PAD;
  return n32 < cap ? n32 : cap;
}

// Kernel by width.  d <= kFusedMaxD: the fused split (syrks_kernel: X staged as fp32
// and split in LDS); above: split pass + half-refill ring (split_kernel,
// syrks_h_kernel).  The fused split re-splits each panel once per tile that reads it
// (~d / 256 times), the split pass once (2 x 4nd bytes), so the split pass's share of
// the op falls as 1/d while the fused split's stays.  Measured (r04, interleaved A/B in
// one process, profiles/r04y_syrk_*_ab.log): config 2, d = 3072, split pass 26.9 vs
// fused 28.8 ms; d = 4096 22.7 vs 25.3; d = 2048 26.10 vs 26.09 - a tie, and the fused
// path needs no image of the shard in the workspace.  (r02, before the half-refill
// ring, profiles/r02l_syrk_fused_ab.log: d = 3072 fused 27.3 vs 29.0 ms; d = 8192
// fused 370 vs 336 ms.)
// The half-refill ring against the K loops it replaced (r04, config-3 shard,
// interleaved A/B in one process, bit-identical, two orders on one box,
// profiles/r04w_syrk_half_ring_ab*.log): 310.6 / 312.6 ms against 316.2 / 319.3 for two
// staggered phases on a whole-K-tile ring and 322.3 / 322.0 for the r03 quarter-refill
// ring: two phases halve the barriers per K-tile and their 48-MFMA M parts cover the L
// parts' DMA issue (four phases 350 / 331 ms, eight 360-366 ms, s_setprio around the
// MFMA clusters 323.5 vs 311.0, profiles/r04t_*, r04u_*), and the half ring gives every
// piece ~1.5 K-tiles of lead instead of one.
constexpr int64_t kFusedMaxD = 2048;

// K-tiles between two flushes of the accumulators, for a call of n rows.
// Two-level fp32 summation: accumulators are added into a per-block slab every
// flush_rows rows.  The error bound ~ (flush_rows / 32 + n / flush_rows) eps is
// smallest at flush_rows ~ sqrt(32 n); each flush is a read-add-write of the block's
// 256 KiB slab beside stalled MFMAs, and the measured error grows slowly above that
// point, so the rule is 2^floor(log2 sqrt(128 n)) within [4096, 16384] (r05,
// interleaved A/B with a float64 check of 64 sampled columns, tools/ab.py syrk,
// profiles/r05z_syrk_flush_ab.log: config-3 shard 8192 -> 16384 rows 314.2 -> 308.6
// ms, max error / max|S| 7.0e-7 -> 8.0e-7; config 2 4096 -> 8192 26.58 -> 25.78 ms,
// 1.9e-7 -> 4.2e-7; 32768 rows at config 3: 305.8 ms but 1.4e-6, config 5's
// n = 65536 at 16384: 2.0e-6 - not taken; r02: 4096 -> 8192 at config 3 337.6 ->
// 331.1 ms, profiles/r02l_syrk_flush.log).
int flush_ktiles(int64_t n) {
#ifdef DEIG_AB_SYRK_FLUSH_ROWS
  int64_t flush_rows = DEIG_AB_SYRK_FLUSH_ROWS;
  (void)n;
#else
  int64_t flush_rows = 4096;
  while (flush_rows < 16384 && (flush_rows * 2) * (flush_rows * 2) <= 128 * n) flush_rows *= 2;
#endif
  return flush_rows < ROWS_PAD ? 1 : (int)(flush_rows / ROWS_PAD);
}

// Everything of the schedule that one call fixes; a pass sets NK and beta (run_pass).
SSched make_sched(const Layout& L, char* base, const float* X, int64_t n, int64_t d, int64_t ldx,
                  float alpha, float* S, int64_t lds) {
  SSched s;
  s.XP = reinterpret_cast<unsigned char*>(base + L.off_xp);
  s.S = S;
  s.part = reinterpret_cast<float*>(base + L.off_part);
  s.accs = reinterpret_cast<float*>(base + L.off_accs);
  s.order = reinterpret_cast<const int*>(base + L.off_order);
  s.lds = lds;
  s.dp = L.dp;
  s.NK = 0;
  s.nseg = (int)L.nseg;
  s.d = (int)d;
  s.nt = (int)L.nt;
  s.T = (int)L.T;
  s.G = (int)L.G;
  s.q = (int)L.q;
  s.R = (int)L.R;
  s.alpha = alpha;
  s.beta = 0;
  s.flush_kt = flush_ktiles(n);
  s.pace = reinterpret_cast<unsigned*>(base + L.off_pace);
  // XCD pacing every 64 K-tiles (2048 rows): config 3 L2 hit rate 0.52 -> 0.75, fabric
  // read requests halved, 345 -> 334 ms (r02, interleaved A/B in one process;
  // 16 / 32 / 128 / 256 K-tiles measured 0.3-1.5 % slower).
  // Remainder rounds of the half ring are paced too (r04, interleaved A/B in one process,
  // profiles/r04za_syrk_*_ab.log, unpaced / paced: config 2 - d = 3072, all 78 tiles
  // remainder - 26.84 / 26.13 ms; d = 4096 22.78 / 22.45; d = 5120 71.8 / 66.7; config-3
  // shard 303.5 / 305.0, within its ~1.5 ms spread): unpaced, the blocks of a remainder
  // round drift apart over their ~2500 K-tiles as the full phases' did.  Numbering the
  // remainder items XCD-major (each XCD's blocks on K ranges no other XCD reads) cost
  // more in balance (nseg a multiple of 8) than it saved in L2 misses (27.15, 23.37,
  // 72.6 ms at the same shapes).
#ifdef DEIG_AB_SYRK_PACE
  s.pace_kt = DEIG_AB_SYRK_PACE;
#else
  s.pace_kt = 64;
#endif
  s.X = X;
  s.ldx = ldx;
  s.nrows = n;
  s.corr = reinterpret_cast<float*>(base + L.off_corr);
  return s;
}

// One pass over s.NK K-tiles: the persistent kernel of this width, the sum of the
// remainder slabs, then the diagonal's lo^2 term from the yb partial rows of s.corr.
int run_pass(const SSched& s, const Layout& L, int64_t yb, hipStream_t stream) {
  if (s.pace_kt > 0) DEIG_HIP_CHECK(hipMemsetAsync(s.pace, 0, 9 * 128, stream));
  if (s.d <= kFusedMaxD)
    hipLaunchKernelGGL(syrks_kernel, dim3((unsigned)L.G), dim3(NTHR), 0, stream, s);
  else
    hipLaunchKernelGGL(syrks_h_kernel, dim3((unsigned)L.G), dim3(NTHR), 0, stream, s);
  DEIG_HIP_CHECK(hipGetLastError());
  if (s.R > 0) {
    hipLaunchKernelGGL(syrks_reduce_kernel, dim3(s.R, SLAB / 4 / 256), dim3(256), 0, stream, s);
    DEIG_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(diag_corr_kernel, dim3((unsigned)cdiv(s.d, 64)), dim3(256), 0, stream, s.corr,
                     (int)yb, L.dp, s.d, s.alpha, s.S, s.lds);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

}  // namespace

// Persistent grid: one block per CU (measurement builds may set a smaller grid, for a
// stream whose CU mask leaves the rest of the chip to other work)
int syrk_cus() {
#ifdef DEIG_AB_SYRK_G
  return DEIG_AB_SYRK_G;
#else
  return num_cus();
#endif
}

size_t syrk_split_workspace_bytes(int64_t n, int64_t d) {
  if (n < 1 || d < 1) return 0;
  return make_layout(d, syrk_cus(), d <= kFusedMaxD ? 0 : default_chunk_rows(n, d)).total;
}

int syrk_split_launch(const float* X, int64_t n, int64_t d, int64_t ldx, float alpha, float* S,
                      int64_t lds, void* ws, size_t ws_bytes, hipStream_t stream, bool accumulate) {
  DEIG_REQUIRE(n >= 1, "syrk: n must be >= 1 (got %lld)", (long long)n);
  DEIG_REQUIRE(d >= 1 && d % 4 == 0, "syrk: d must be a positive multiple of 4 (got %lld)",
               (long long)d);
  DEIG_REQUIRE(d <= (1 << 16) - BT, "syrk: d too large (%lld)", (long long)d);
  DEIG_REQUIRE(ldx >= d && ldx % 4 == 0, "syrk: ldx must be >= d and a multiple of 4");
  DEIG_REQUIRE(lds >= d && lds % 4 == 0, "syrk: lds must be >= d and a multiple of 4");
  DEIG_REQUIRE(X && S && aligned16(X) && aligned16(S), "syrk: X and S must be 16-byte aligned");
  const int G = syrk_cus();
  const bool fused = d <= kFusedMaxD;
  // Largest chunk (multiple of 32 rows, <= n rounded up) that fits the workspace.
  const Layout L0 = make_layout(d, G, 0);
  const size_t ws_min = L0.total + (fused ? 0 : (size_t)ROWS_PAD * L0.dp * 4);
  if (!ws || ws_bytes < ws_min)
    return fail(DEIG_EWORKSPACE, "syrk: workspace %zu bytes < minimum %zu", ws_bytes, ws_min);
  int64_t chunk = (int64_t)((ws_bytes - L0.total) / (size_t)(L0.dp * 4)) / ROWS_PAD * ROWS_PAD;
  const int64_t n32 = cdiv(n, ROWS_PAD) * ROWS_PAD;
  if (chunk > n32) chunk = n32;
  const Layout L = make_layout(d, G, fused ? 0 : chunk);
  char* base = static_cast<char*>(ws);
  SSched s = make_sched(L, base, X, n, d, ldx, alpha, S, lds);
  if (G == 256 && s.nt % 8 == 0)
    hipLaunchKernelGGL(tile_order_compact_kernel, dim3((unsigned)cdiv((s.nt / 8) * (s.nt / 8), 256)), dim3(256), 0,
                       stream, s.nt, reinterpret_cast<int*>(base + L.off_order));
  else
    hipLaunchKernelGGL(tile_order_kernel,
                       dim3((unsigned)cdiv(cdiv(s.nt, SUPER_H) * cdiv(s.nt, SUPER_W), 256)), dim3(256), 0, stream,
                       s.nt, reinterpret_cast<int*>(base + L.off_order));
  DEIG_HIP_CHECK(hipGetLastError());
  if (fused) {
    DEIG_REQUIRE(ldx <= (int64_t(1) << 25), "syrk: ldx > 2^25 is not supported for d <= 2048");
    // One pass over all n rows (no XP image, no chunks).  lo^2 partials:
    // [segment < max(1, nseg)][octet wave < 4][dp], zero where no diagonal tile wrote.
    const int64_t yb = 4 * (L.nseg > 1 ? L.nseg : 1);
    DEIG_REQUIRE(yb <= L.yb_max, "syrk: %lld lo^2 partial rows exceed the workspace's %lld",
                 (long long)yb, (long long)L.yb_max);
    DEIG_HIP_CHECK(hipMemsetAsync(s.corr, 0, sizeof(float) * (size_t)(yb * L.dp), stream));
    s.NK = cdiv(n, ROWS_PAD);
    s.beta = accumulate ? 1 : 0;
    return run_pass(s, L, yb, stream);
  }
  for (int64_t r0 = 0, c = 0; r0 < n; r0 += chunk, ++c) {
    const int64_t rows = (n - r0) < chunk ? (n - r0) : chunk;
    const int64_t nk = cdiv(rows, ROWS_PAD);  // K-tiles = 32-row blocks (zero-padded)
    const int64_t noct = nk * (ROWS_PAD / 8);
    int64_t yb = cdiv(noct, 4);
    if (yb > L.yb_max) yb = L.yb_max;
    hipLaunchKernelGGL(split_kernel, dim3((unsigned)(L.dp / 256), (unsigned)yb), dim3(256), 0,
                       stream, X + r0 * ldx, rows, ldx, (int)d, L.dp, noct, s.XP, s.corr);
    DEIG_HIP_CHECK(hipGetLastError());
    s.NK = nk;
    s.beta = (c > 0 || accumulate) ? 1 : 0;
    if (int rc = run_pass(s, L, yb, stream)) return rc;
  }
  return DEIG_OK;
}

}  // namespace deig
