// Scaling of hourly fields: box moments over space and time.  hourly [n][24][ny][nx] fp32 with a day stride.
// q = rd_depth_q(x) in 1/1024 mm, a pixel-hour is bad under rd_depth_bad.  Space level a = 0 .. A: boxes of 2^a x 2^a pixels on the
// dyadic grid anchored at pixel (0, 0), only those wholly inside the plane; time level b = 0 .. 4: aligned windows of 1, 2, 4, 8, 24
// hours of the day.  R is the sum of q over a box and a window, and a box-window that holds a bad pixel-hour is void.  The state is
// one record of RD_SC_REC words per (a, b) at (a * 5 + b) * RD_SC_REC, in the order of the RD_SC_* offsets below, then n_days_total
// and n_bad.
//
//  * k_scaling_tiles: a workgroup of 4 waves takes units in a grid-stride loop; a unit is a 64 x 64 block of one day, or, for a plane
//    narrower or lower than 64, the collage of 64 / 2^lbh x 64 / 2^lbw days whose shares (the sides padded to powers of two) fill
//    the block -- nd 16 puts 16 days into a unit.  A share is aligned to its own size, so the dyadic boxes of the block are those
//    of the planes up to the level the plane admits.
//    A thread holds cell (cy, cx) of the 16 x 16 cells, 4 x 4 pixels, its lane the Morton code of the cell inside the wave's 8 x 8
//    cells: levels 0 .. 2 are sums inside the thread, levels 3 .. 5 two xor shuffles each of (R | bad << 40), level 6 is the sum of
//    the four waves' totals through LDS.  The thread walks the 24 hours once, the next hour's values in flight while this hour is
//    counted; it carries the 2-, 4-, 8- and 24-hour sums of its 16 pixels with a mask of the bad ones, and when a window closes
//    (the conditions are nested: a closing window closes every shorter one) its sums go through the space levels.
//    Per level the wave counts its dry boxes with ballots of the bits of the lanes' counts (bin 0 takes no LDS atomic), a wet box is
//    one 32-bit LDS atomic on its bin; the lanes' sum1 and the three words of the second moment are summed over the wave (four DPP
//    row rotations and two shuffles per word) and lane 0 adds them to the workgroup's words in LDS -- skipped by a wave with no wet
//    box at that level.  The maximum is compared with the word in LDS first (it only grows, so a stale read costs an atomic and
//    never loses one).  At the end every non-zero counter goes to the state with one 64-bit integer atomic; n_boxes and n_wet are
//    sums of the histogram.
// The 32-bit counters: a unit adds at most 64 * 64 * 24 < 2^17 to one of them and a workgroup takes fewer than 2^15 units (the
// entry sizes the grid so).  No floating point behind the quantisation, no floating-point atomics, no spin-waits, no grid sync.
// All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_SC_THREADS 256
#define RD_SC_TILE 64                    // side of a unit in pixels
#define RD_SC_MAXA 6                     // the largest space level: one box per unit
#define RD_SC_NT 5                       // time levels: windows of 1, 2, 4, 8, 24 hours
#define RD_SC_BINS 288                   // bins of R: 0, 1 .. 7, then eight per octave up to 2^38
#define RD_SC_SPLIT 19                   // R = h * 2^19 + l in the second moment
// the words of a record
#define RD_SC_NBOXES 0
#define RD_SC_NVOID 1
#define RD_SC_NWET 2
#define RD_SC_SUM1 3
#define RD_SC_SUM2_HH 4
#define RD_SC_SUM2_HL 5
#define RD_SC_SUM2_LL 6
#define RD_SC_MAX_R 7
#define RD_SC_HIST 8
#define RD_SC_REC (RD_SC_HIST + RD_SC_BINS)
#define RD_SC_MAXREC ((RD_SC_MAXA + 1) * RD_SC_NT)
#define RD_SC_WORKSPACE 8                // bytes: nothing is held back, the size stands for "a workspace"
#define RD_SC_MINGRID 2048               // workgroups of a launch with that many units or more
#define RD_SC_MAXUNITS 32768             // units one workgroup may take: its 32-bit counters hold 2^32 / (64 * 64 * 24) = 43690

inline long rd_sc_state_count(int A) { return (long)(A + 1) * RD_SC_NT * RD_SC_REC + 2; }

// the geometry of a call: the blocks and the collage
struct rd_sc_geo {
  int ny, nx, A;
  int lbh, lbw;                          // log2 of a day's share of the block: 6 where the side has 64 pixels or more
  int nby, nbx;                          // blocks of a plane
  int G;                                 // days of a collage: (64 >> lbh) * (64 >> lbw)
};

inline int rd_sc_log2_ceil(long n) {
  int l = 0;
  while ((1L << l) < n) ++l;
  return l;
}

inline rd_sc_geo rd_sc_geometry(long ny, long nx, int A) {
  rd_sc_geo g;
  g.ny = (int)ny, g.nx = (int)nx, g.A = A;
  g.lbh = ny >= RD_SC_TILE ? 6 : rd_sc_log2_ceil(ny), g.lbw = nx >= RD_SC_TILE ? 6 : rd_sc_log2_ceil(nx);
  g.nby = (int)((ny + RD_SC_TILE - 1) / RD_SC_TILE), g.nbx = (int)((nx + RD_SC_TILE - 1) / RD_SC_TILE);
  g.G = (RD_SC_TILE >> g.lbh) * (RD_SC_TILE >> g.lbw);
  return g;
}

// the bin of R: 0, 1 .. 7, then 8 + 8 (e - 3) + the three bits below the leading one, e = floor(log2 R)
__device__ __forceinline__ int rd_sc_bin(unsigned long long R) {
  if (R < 8ull) return (int)R;
  const int e = 63 - __clzll((long long)R);
  return 8 + 8 * (e - 3) + (int)((R >> (e - 3)) & 7ull);
}

__device__ __forceinline__ int rd_sc_even_bits(int v) { return (v & 1) | ((v >> 1) & 2) | ((v >> 2) & 4); }

__device__ __forceinline__ unsigned long long rd_sc_shfl_xor64(unsigned long long v, int k) {
  const unsigned lo = __shfl_xor((unsigned)v, k), hi = __shfl_xor((unsigned)(v >> 32), k);
  return ((unsigned long long)hi << 32) | lo;
}

// the sum of v over the wave, in every lane: the rows of 16 by DPP rotations, the four rows by two shuffles
template <int CTRL> __device__ __forceinline__ unsigned long long rd_sc_dpp64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long rd_sc_wave_sum(unsigned long long v) {
  v += rd_sc_dpp64<0x128>(v);                                                  // row_ror:8, 4, 2, 1
  v += rd_sc_dpp64<0x124>(v);
  v += rd_sc_dpp64<0x122>(v);
  v += rd_sc_dpp64<0x121>(v);
  v += rd_sc_shfl_xor64(v, 16);
  v += rd_sc_shfl_xor64(v, 32);
  return v;
}

// the sum over the wave of the lanes' counts c < 2^BITS: one ballot per bit
template <int BITS> __device__ __forceinline__ unsigned rd_sc_wave_count(unsigned c) {
  unsigned n = 0;
#pragma unroll
  for (int k = 0; k < BITS; ++k) n += (unsigned)__popcll(__ballot((c >> k) & 1u)) << k;
  return n;
}

// what a lane adds to a record: the sums over its own valid wet boxes
struct rd_sc_sums {
  unsigned long long s1, hh, hl, ll, mx;
};
__device__ __forceinline__ void rd_sc_take(rd_sc_sums& s, unsigned long long R) {
  const unsigned h = (unsigned)(R >> RD_SC_SPLIT), l = (unsigned)R & ((1u << RD_SC_SPLIT) - 1u);
  s.s1 += R;
  s.hh += (unsigned long long)h * h, s.hl += (unsigned long long)h * l, s.ll += (unsigned long long)l * l;
  s.mx = R > s.mx ? R : s.mx;
}

// the words of a record the workgroup keeps in LDS besides the histogram
#define RD_SC_L_NVOID 0
#define RD_SC_L_SUM1 1
#define RD_SC_L_HH 2
#define RD_SC_L_HL 3
#define RD_SC_L_LL 4
#define RD_SC_L_MAX 5
#define RD_SC_L_WORDS 6

// one level of one window for a wave: n_dry and n_void are the wave's counts (uniform), s the lane's sums
__device__ __forceinline__ void rd_sc_wave_add(unsigned* hist, unsigned long long* fix, int lane, unsigned n_dry, unsigned n_void,
                                               const rd_sc_sums& s) {
  if (lane == 0) {
    if (n_dry) atomicAdd(&hist[0], n_dry);
    if (n_void) atomicAdd(&fix[RD_SC_L_NVOID], (unsigned long long)n_void);
  }
  if (__ballot(s.s1 != 0ull) == 0ull) return;                                 // (the whole wave)
  const unsigned long long s1 = rd_sc_wave_sum(s.s1), hh = rd_sc_wave_sum(s.hh), hl = rd_sc_wave_sum(s.hl), ll = rd_sc_wave_sum(s.ll);
  if (lane == 0) {
    atomicAdd(&fix[RD_SC_L_SUM1], s1);
    if (hh) atomicAdd(&fix[RD_SC_L_HH], hh);
    if (hl) atomicAdd(&fix[RD_SC_L_HL], hl);
    atomicAdd(&fix[RD_SC_L_LL], ll);
  }
  if (s.mx > fix[RD_SC_L_MAX]) atomicMax(&fix[RD_SC_L_MAX], s.mx);
}

// one box of a lane: counted (wholly inside the plane of a day the call holds), bad (void), R
__device__ __forceinline__ void rd_sc_box(unsigned* hist, bool counted, bool bad, unsigned long long R, unsigned& n_dry, unsigned& n_void,
                                          rd_sc_sums& s) {
  n_void += counted && bad;
  const bool valid = counted && !bad;
  n_dry += valid && R == 0ull;
  if (valid && R != 0ull) {
    rd_sc_take(s, R);
    atomicAdd(&hist[rd_sc_bin(R)], 1u);
  }
}

// grid (workgroups), units in a grid-stride loop.  unit = day group * (nby nbx) + block of the plane.  V = 4: 16-byte loads, every
// row of every day on 16 bytes and nx a multiple of 4 (rd_vec4_ok)
template <int V>
__global__ void __launch_bounds__(RD_SC_THREADS)
k_scaling_tiles(const float* __restrict__ hourly, long n, long day_stride, rd_sc_geo g, long units, unsigned long long* __restrict__ counts) {
  __shared__ unsigned hist[RD_SC_MAXREC][RD_SC_BINS];
  __shared__ unsigned long long fix[RD_SC_MAXREC][RD_SC_L_WORDS];
  __shared__ unsigned long long tot[RD_SC_MAXREC][2];                          // n_boxes, n_wet: sums of the histogram
  __shared__ unsigned long long w5[2][4];                                      // the waves' level-5 totals, two windows in turn
  __shared__ unsigned long long bad_total;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = g.A;
  const int nrec = (A + 1) * RD_SC_NT;
  const long plane = (long)g.ny * g.nx;
  constexpr int NOFF = V == 4 ? 4 : 16;

  for (int i = tid; i < RD_SC_MAXREC * RD_SC_BINS; i += RD_SC_THREADS) (&hist[0][0])[i] = 0u;
  for (int i = tid; i < RD_SC_MAXREC * RD_SC_L_WORDS; i += RD_SC_THREADS) (&fix[0][0])[i] = 0ull;
  for (int i = tid; i < RD_SC_MAXREC * 2; i += RD_SC_THREADS) (&tot[0][0])[i] = 0ull;
  if (tid == 0) bad_total = 0ull;
  __syncthreads();

  // this thread's cell: rows 4 cy .., columns 4 cx .. of the block
  const int cx = rd_sc_even_bits(lane) | ((wave & 1) << 3), cy = rd_sc_even_bits(lane >> 1) | ((wave >> 1) << 3);
  const int shares_x = RD_SC_TILE >> g.lbw, mh = (1 << g.lbh) - 1, mw = (1 << g.lbw) - 1;
  const long blocks = (long)g.nby * g.nbx;
  unsigned n_bad = 0;
  int parity = 0;                                                              // of the windows that reached level 6

  for (long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int blk = (int)(unit % blocks);
    const int y0 = blk / g.nbx * RD_SC_TILE, x0 = blk % g.nbx * RD_SC_TILE;
    const long day0 = unit / blocks * g.G;
    // the pixel (r, c) of the block: inside the plane of a day the call holds?  and where
    auto pixel = [&](int r, int c, long* off) {
      const int y = y0 + (r & mh), x = x0 + (c & mw);
      const long day = day0 + (r >> g.lbh) * shares_x + (c >> g.lbw);
      *off = day * day_stride + (long)y * g.nx + x;
      return y < g.ny && x < g.nx && day < n;
    };
    // the box of side 2^a that holds the pixel (r, c): wholly inside?  (its last pixel is; a <= lbh, lbw keeps it in one share)
    auto inside = [&](int a, int r, int c) {
      long unused;
      const int s = (1 << a) - 1;
      return pixel(r | s, c | s, &unused);
    };
    long off[NOFF];
    unsigned in16 = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      long o;
      in16 |= (unsigned)pixel(4 * cy + (i >> 2), 4 * cx + (i & 3), &o) << i;
      if constexpr (V == 4) {
        if ((i & 3) == 0) off[i >> 2] = o;
      } else {
        off[i] = o;
      }
    }
    // the boxes this thread counts: bits 0 .. 3 the four 2 x 2 boxes of the cell, bit 4 the cell, bits 5 .. 8 levels 3 .. 6
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt |= (unsigned)inside(1, 4 * cy + 2 * (k >> 1), 4 * cx + 2 * (k & 1)) << k;
    cnt |= (unsigned)inside(2, 4 * cy, 4 * cx) << 4;
    cnt |= (unsigned)((lane & 3) == 0 && inside(3, 4 * cy, 4 * cx)) << 5;
    cnt |= (unsigned)((lane & 15) == 0 && inside(4, 4 * cy, 4 * cx)) << 6;
    cnt |= (unsigned)(lane == 0 && inside(5, 4 * cy, 4 * cx)) << 7;
    cnt |= (unsigned)(tid == 0 && inside(6, 0, 0)) << 8;

    auto load = [&](int h, float (&v)[16]) {
      const float* src = hourly + h * plane;
#pragma unroll
      for (int i = 0; i < 16; i += V) {
        if ((in16 >> i) & 1u) {
          float t[V];
          rd_load<V>(src + off[i / V], t);
#pragma unroll
          for (int j = 0; j < V; ++j) v[i + j] = t[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) v[i + j] = 0.0f;
        }
      }
    };

    unsigned a2[16], a4[16], a8[16], a24[16];
    unsigned b2 = 0, b4 = 0, b8 = 0, b24 = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) a2[i] = a4[i] = a8[i] = a24[i] = 0u;
    float next[16];
    load(0, next);

#pragma unroll 1
    for (int h = 0; h < RD_HOURS; ++h) {
      unsigned q[16], b1 = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool bad = ((in16 >> i) & 1u) && rd_depth_bad(next[i]);
        b1 |= (unsigned)bad << i;
        q[i] = bad ? 0u : (unsigned)rd_depth_q(next[i]);
      }
      if (h + 1 < RD_HOURS) load(h + 1, next);
      n_bad += __popc(b1);
      b2 |= b1, b4 |= b1, b8 |= b1, b24 |= b1;
#pragma unroll
      for (int i = 0; i < 16; ++i) a2[i] += q[i], a4[i] += q[i], a8[i] += q[i], a24[i] += q[i];

#pragma unroll 1
      for (int b = 0; b < RD_SC_NT; ++b) {
        // the windows that close behind hour h: 1 hour always, 2, 4, 8 hours at their last hour, the day at hour 23
        if (b > 0 && !(b < 4 ? (h & ((1 << b) - 1)) == (1 << b) - 1 : h == RD_HOURS - 1)) break;
        unsigned t[16], tb;
        if (b == 0) {
          tb = b1;
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = q[i];
        } else if (b == 1) {
          tb = b2, b2 = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = a2[i], a2[i] = 0u;
        } else if (b == 2) {
          tb = b4, b4 = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = a4[i], a4[i] = 0u;
        } else if (b == 3) {
          tb = b8, b8 = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = a8[i], a8[i] = 0u;
        } else {
          tb = b24, b24 = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = a24[i], a24[i] = 0u;
        }
        const bool wave_bad = __ballot(tb != 0u) != 0ull;                     // (no void box in the wave's levels 0 .. 5 otherwise)

        // level 0: the 16 pixels
        {
          unsigned wet = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) wet |= (unsigned)(t[i] != 0u) << i;
          const unsigned valid = in16 & ~tb;
          wet &= valid;
          const unsigned n_dry = rd_sc_wave_count<5>(__popc(valid & ~wet));
          const unsigned n_void = wave_bad ? rd_sc_wave_count<5>(__popc(in16 & tb)) : 0u;
          rd_sc_sums s = {};
          if (wet) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if ((wet >> i) & 1u) {
                rd_sc_take(s, t[i]);
                atomicAdd(&hist[b][rd_sc_bin(t[i])], 1u);
              }
          }
          rd_sc_wave_add(hist[b], fix[b], lane, n_dry, n_void, s);
        }
        if (A < 1) continue;
        // level 1: the four 2 x 2 boxes of the cell
        unsigned r1[4];
        {
          unsigned n_dry = 0, n_void = 0;
          rd_sc_sums s = {};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int i0 = 8 * (k >> 1) + 2 * (k & 1);
            const unsigned mk = 0x33u << i0;
            r1[k] = t[i0] + t[i0 + 1] + t[i0 + 4] + t[i0 + 5];
            rd_sc_box(hist[RD_SC_NT + b], (cnt >> k) & 1u, (tb & mk) != 0u, r1[k], n_dry, n_void, s);
          }
          rd_sc_wave_add(hist[RD_SC_NT + b], fix[RD_SC_NT + b], lane, rd_sc_wave_count<3>(n_dry), wave_bad ? rd_sc_wave_count<3>(n_void) : 0u, s);
        }
        if (A < 2) continue;
        // level 2: the cell
        const unsigned r2 = r1[0] + r1[1] + r1[2] + r1[3];
        {
          unsigned n_dry = 0, n_void = 0;
          rd_sc_sums s = {};
          rd_sc_box(hist[2 * RD_SC_NT + b], (cnt >> 4) & 1u, tb != 0u, r2, n_dry, n_void, s);
          rd_sc_wave_add(hist[2 * RD_SC_NT + b], fix[2 * RD_SC_NT + b], lane, rd_sc_wave_count<1>(n_dry), wave_bad ? rd_sc_wave_count<1>(n_void) : 0u, s);
        }
        if (A < 3) continue;
        // levels 3 .. 5: 4, 16, 64 lanes; the bad cells are counted above bit 40 (R < 2^38)
        unsigned long long val = (unsigned long long)r2 | ((unsigned long long)(tb != 0u) << 40);
#pragma unroll 1
        for (int a = 3; a <= 5 && a <= A; ++a) {
          val += rd_sc_shfl_xor64(val, 1 << (2 * (a - 3)));
          val += rd_sc_shfl_xor64(val, 2 << (2 * (a - 3)));
          const int rec = a * RD_SC_NT + b;
          unsigned n_dry = 0, n_void = 0;
          rd_sc_sums s = {};
          rd_sc_box(hist[rec], (cnt >> (a + 2)) & 1u, (val >> 40) != 0ull, val & ((1ull << 40) - 1ull), n_dry, n_void, s);
          rd_sc_wave_add(hist[rec], fix[rec], lane, rd_sc_wave_count<1>(n_dry), wave_bad ? rd_sc_wave_count<1>(n_void) : 0u, s);
        }
        if (A < 6) continue;
        // level 6: the block, by thread 0 from the four waves' totals
        if (lane == 0) w5[parity][wave] = val;
        __syncthreads();
        if (tid == 0) {
          const unsigned long long v6 = w5[parity][0] + w5[parity][1] + w5[parity][2] + w5[parity][3];
          const unsigned long long R = v6 & ((1ull << 40) - 1ull);
          const int rec = 6 * RD_SC_NT + b;
          if ((cnt >> 8) & 1u) {
            if (v6 >> 40) {
              atomicAdd(&fix[rec][RD_SC_L_NVOID], 1ull);
            } else if (R == 0ull) {
              atomicAdd(&hist[rec][0], 1u);
            } else {
              rd_sc_sums s = {};
              rd_sc_take(s, R);
              atomicAdd(&hist[rec][rd_sc_bin(R)], 1u);
              atomicAdd(&fix[rec][RD_SC_L_SUM1], s.s1);
              atomicAdd(&fix[rec][RD_SC_L_HH], s.hh);
              atomicAdd(&fix[rec][RD_SC_L_HL], s.hl);
              atomicAdd(&fix[rec][RD_SC_L_LL], s.ll);
              atomicMax(&fix[rec][RD_SC_L_MAX], R);
            }
          }
        }
        parity ^= 1;
      }
    }
  }

  // the workgroup's counters to the state
  {
    const unsigned long long nb = rd_sc_wave_sum((unsigned long long)n_bad);
    if (lane == 0 && nb) atomicAdd(&bad_total, nb);
  }
  __syncthreads();
  for (int rec = 0; rec < nrec; ++rec) {
    const unsigned c0 = hist[rec][tid], c1 = tid < RD_SC_BINS - RD_SC_THREADS ? hist[rec][RD_SC_THREADS + tid] : 0u;
    unsigned long long* out = counts + (long)rec * RD_SC_REC + RD_SC_HIST;
    if (c0) atomicAdd(&out[tid], (unsigned long long)c0);
    if (c1) atomicAdd(&out[RD_SC_THREADS + tid], (unsigned long long)c1);
    const unsigned long long all = rd_sc_wave_sum((unsigned long long)c0 + c1);
    const unsigned long long wet = rd_sc_wave_sum((unsigned long long)(tid == 0 ? 0u : c0) + c1);
    if (lane == 0) {
      if (all) atomicAdd(&tot[rec][0], all);
      if (wet) atomicAdd(&tot[rec][1], wet);
    }
  }
  __syncthreads();
  for (int i = tid; i < nrec * RD_SC_HIST; i += RD_SC_THREADS) {
    const int rec = i / RD_SC_HIST, w = i % RD_SC_HIST;
    unsigned long long* out = counts + (long)rec * RD_SC_REC + w;
    const unsigned long long v = w == RD_SC_NBOXES ? tot[rec][0] : w == RD_SC_NWET ? tot[rec][1] : fix[rec][w == RD_SC_NVOID ? RD_SC_L_NVOID : w - 2];
    if (!v) continue;
    if (w == RD_SC_MAX_R) atomicMax(out, v);
    else atomicAdd(out, v);
  }
  unsigned long long* tail = counts + (long)nrec * RD_SC_REC;                  // n_days_total, n_bad
  if (tid == 0) {
    if (blockIdx.x == 0) atomicAdd(&tail[0], (unsigned long long)n);
    if (bad_total) atomicAdd(&tail[1], bad_total);
  }
}
