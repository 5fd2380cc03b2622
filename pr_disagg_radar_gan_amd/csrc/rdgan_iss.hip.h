// Scale-separation verification of hourly fields: the integer state of the intensity-scale skill score
// (Casati, Ross and Stephenson 2004).  members [s][n_days][24][ny][nx] fp32 with a member stride, obs [n_days][24][ny][nx] dense.
// For a threshold u the event of a finite value v is v > u in fp32; a tile is a square of side 2^L, the plane is cropped (centred)
// to whole tiles, and a tile of a pair (member plane, observed plane) is void when any of its pixels is NaN or +-inf on either
// side.  With SX_l(b), SO_l(b) the events of the member and of the observation in the block b of side 2^l, the state is
//   counts[t][h][l][3] = sum over the valid tiles of all pairs of (SX_l^2, SO_l^2, SX_l SO_l), l = 0 .. L;  tiles[h][2] = (valid, void)
//
//  * k_iss_tiles: a workgroup of 4 waves owns a 64 x 64 block of the cropped plane of one (day, hour).  A wave packs 16 rows: the
//    ballot of a compare of 64 adjacent pixels is the row's word.  The observation's words are formed once, cut into the 16-bit
//    cell (4 x 4 pixels) each thread owns and kept in LDS; the workgroup then loops over its members.  The member's values of the
//    next round are loaded while this round is computed; its words lie in LDS twice, so a round costs one barrier.
//    A thread holds cell (cy, cx) of the 16 x 16 cells, its index the Morton code of (cy, cx): levels 0 .. 2 are popcounts of the
//    cell under masks, level 3 is the sum over 4 adjacent lanes, level 4 over 16, level 5 over the wave, all by xor shuffles of
//    the packed (SX, SO).  The squares and products of levels 0 .. 3 travel in three 64-bit words of four fields (12, 14, 16, 18
//    bits: a wave's sums fit), those of level 4 in one of three 20-bit fields, and are summed over the wave by the same shuffles;
//    lane 0 adds them to the workgroup's counters in LDS.  Level 6 (L = 6) is wave 0's: a lane per row word.
//    The void rule clears the cell's bits of a void tile before anything is counted: the flag of a tile is the OR of the cells'
//    bad bits over 4^(L - 2) adjacent lanes (L = 1: per 2 x 2 inside the cell; L >= 6: over the four waves through LDS).
//    A plane narrower or lower than 64 is padded to the next power of two, and the block takes 64 / that many days of the same
//    hour side by side (a collage): nd 16 fills a block with 16 days, no lane idles where there are days enough.
//    At the end a thread adds one non-zero counter to the state with a 64-bit integer atomic.
//  * L = 7 .. 10: k_iss_tiles clears nothing across blocks; it writes per (pair, block, threshold, wave) the wave's 18 sums of levels
//    0 .. 5 and its (SX_5, SO_5) into the workspace, and per (pair, block) a bad flag: the sums are HELD BACK.  k_iss_upper, one
//    workgroup per (pair, tile), drops a tile with a flagged block and otherwise adds the held sums, forms level 6 from the four
//    waves' totals and levels 7 .. L by summing four Morton neighbours at a time in LDS.
// No floating-point atomics, no spin-waits, no grid sync.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_ISS_MAXT RD_THR_MAX
#define RD_ISS_MAXL 10
#define RD_ISS_MAXS 4096
#define RD_ISS_THREADS 256
#define RD_ISS_BLOCK 64                  // side of a workgroup's block in pixels
#define RD_ISS_REC 20                    // 32-bit words of a wave's record: 18 sums of levels 0 .. 5, SX_5, SO_5
#define RD_ISS_MAXUNITS 65535            // (day group, hour) units of one launch: gridDim.y
#define RD_ISS_MAXSPLIT 64               // member slices of one launch: gridDim.z

// the geometry of a call: the crop, the blocks and the collage
struct rd_iss_geo {
  int ny, nx, L;
  int oy, ox, cy, cx;                    // the crop: offset and size, multiples of 2^L
  int lbh, lbw;                          // log2 of a day's share of the block: 6 where the crop has 64 pixels or more
  int nby, nbx;                          // blocks of a plane
  int G;                                 // days of a collage: (64 >> lbh) * (64 >> lbw)
};

inline int rd_iss_log2_ceil(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

inline rd_iss_geo rd_iss_geometry(long ny, long nx, int L) {
  rd_iss_geo g;
  const int side = 1 << L;
  g.ny = (int)ny, g.nx = (int)nx, g.L = L;
  g.cy = (int)(ny / side) * side, g.cx = (int)(nx / side) * side;
  g.oy = (int)(ny % side) / 2, g.ox = (int)(nx % side) / 2;
  g.lbh = g.cy >= RD_ISS_BLOCK ? 6 : rd_iss_log2_ceil(g.cy), g.lbw = g.cx >= RD_ISS_BLOCK ? 6 : rd_iss_log2_ceil(g.cx);
  g.nby = (g.cy + RD_ISS_BLOCK - 1) / RD_ISS_BLOCK, g.nbx = (g.cx + RD_ISS_BLOCK - 1) / RD_ISS_BLOCK;
  g.G = (RD_ISS_BLOCK >> g.lbh) * (RD_ISS_BLOCK >> g.lbw);
  return g;
}

// bytes of the workspace one pair takes: nothing is held back up to L = 6 (8 bytes stand for "a workspace"); above, per block
// RD_ISS_MAXT thresholds x 4 waves x RD_ISS_REC words and the flag
inline long rd_iss_pair_bytes(long ny, long nx, int L) {
  if (L <= 6) return 8;
  const rd_iss_geo g = rd_iss_geometry(ny, nx, L);
  return (long)g.nby * g.nbx * (RD_ISS_MAXT * 4 * RD_ISS_REC * 4 + 8);
}

// the Morton code of lane bits: even bits -> x, odd bits -> y (3 bits each)
__device__ __forceinline__ int rd_iss_even_bits(int v) { return (v & 1) | ((v >> 1) & 2) | ((v >> 2) & 4); }

// the pixel (r, c) of a workgroup's block: is it inside the crop of a day the call holds, and where does it lie
struct rd_iss_block {
  int y0, x0;                            // the block's corner in the crop
  long day0;                             // the first day of the collage
  long n_days;
};
__device__ __forceinline__ bool rd_iss_pixel(const rd_iss_geo& g, const rd_iss_block& b, long day_elems, long plane_off, int r, int c,
                                             long* off) {
  const int jy = r >> g.lbh, jx = c >> g.lbw;
  const int y = b.y0 + (r & ((1 << g.lbh) - 1)), x = b.x0 + (c & ((1 << g.lbw) - 1));
  const long day = b.day0 + jy * (RD_ISS_BLOCK >> g.lbw) + jx;
  *off = day * day_elems + plane_off + (long)(g.oy + y) * g.nx + g.ox + x;
  return y < g.cy && x < g.cx && day < b.n_days;
}

// the 16 bits of cell (cy, cx) out of four row words
__device__ __forceinline__ unsigned rd_iss_cell(const unsigned long long* words, int cy, int cx) {
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) v |= (unsigned)((words[4 * cy + i] >> (4 * cx)) & 0xFull) << (4 * i);
  return v;
}

__device__ __forceinline__ unsigned long long rd_iss_shfl_xor64(unsigned long long v, int k) {
  const unsigned lo = __shfl_xor((unsigned)v, k), hi = __shfl_xor((unsigned)(v >> 32), k);
  return ((unsigned long long)hi << 32) | lo;
}

// grid (blocks of a plane, units of the launch, member slices).  unit u0 + blockIdx.y = day group * 24 + hour; the members
// m0 .. m0 + nm - 1 of the call are cut into gridDim.z slices.  held (L > 6): the records [pair][block][t][wave][RD_ISS_REC] with
// pair = (m - m0) * units + blockIdx.y, and flags [pair][block] behind them
__global__ void __launch_bounds__(RD_ISS_THREADS)
k_iss_tiles(const float* __restrict__ members, long member_stride, int m0, int nm, const float* __restrict__ obs, long n_days,
            rd_iss_geo g, rd_thr thr, int T, long u0, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ tiles,
            unsigned* __restrict__ held, unsigned* __restrict__ held_flags) {
  __shared__ unsigned long long words[2][RD_ISS_MAXT + 1][RD_ISS_BLOCK];       // [buffer][bad, event t][row]
  __shared__ unsigned cell_o[RD_ISS_MAXT][RD_ISS_THREADS];                     // the observation's cell of every thread
  __shared__ unsigned long long cnt[RD_ISS_MAXT][7][3];
  __shared__ unsigned so6[RD_ISS_MAXT];
  __shared__ unsigned wave_bad[2][4];
  __shared__ unsigned tile_cnt[2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = g.L;
  const long unit = u0 + blockIdx.y;
  const int hour = (int)(unit % RD_HOURS);
  const long plane = (long)g.ny * g.nx, day_elems = RD_HOURS * plane, plane_off = hour * plane;
  rd_iss_block b;
  b.y0 = (int)(blockIdx.x / g.nbx) * RD_ISS_BLOCK, b.x0 = (int)(blockIdx.x % g.nbx) * RD_ISS_BLOCK;
  b.day0 = unit / RD_HOURS * g.G, b.n_days = n_days;
  // the members of this slice
  const int per = (nm + (int)gridDim.z - 1) / (int)gridDim.z;
  const int ma = m0 + (int)blockIdx.z * per, mb = min(m0 + nm, ma + per);
  if (ma >= mb) return;                                                       // (the whole workgroup)

  for (int i = tid; i < RD_ISS_MAXT * 7 * 3; i += RD_ISS_THREADS) (&cnt[0][0][0])[i] = 0ull;
  if (tid < 2) tile_cnt[tid] = 0u;

  // the 16 pixels of this thread's loads: row wave * 16 + i, column lane
  long off[16];
  unsigned in_rows = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) in_rows |= (unsigned)rd_iss_pixel(g, b, day_elems, plane_off, wave * 16 + i, lane, &off[i]) << i;

  // pack 16 rows of values into words[buf]: lane 0 keeps the bad word, lane 1 + t the events of threshold t
  auto pack = [&](const float (&v)[16], int buf) {
    unsigned any_bad = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool in = (in_rows >> i) & 1u;
      unsigned long long mine = __ballot(in && rd_nonfinite(v[i]));
      any_bad |= mine != 0ull;
#pragma unroll
      for (int t = 0; t < RD_ISS_MAXT; ++t)
        if (t < T) {
          const unsigned long long e = __ballot(in && v[i] > thr.v[t]);
          mine = lane == t + 1 ? e : mine;
        }
      if (lane <= T) words[buf][lane][wave * 16 + i] = mine;
    }
    if (lane == 0) wave_bad[buf][wave] = any_bad;
  };
  auto load = [&](const float* src, float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (in_rows >> i) & 1u ? src[off[i]] : 0.0f;
  };

  // this thread's cell
  const int cx = rd_iss_even_bits(lane) | ((wave & 1) << 3), cy = rd_iss_even_bits(lane >> 1) | ((wave >> 1) << 3);
  unsigned in16 = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    long unused;
    in16 |= (unsigned)rd_iss_pixel(g, b, day_elems, plane_off, 4 * cy + (i >> 2), 4 * cx + (i & 3), &unused) << i;
  }

  float v[16];
  load(obs, v);
  pack(v, 0);
  load(members + (long)ma * member_stride, v);
  __syncthreads();
  const unsigned bad_o16 = rd_iss_cell(words[0][0], cy, cx);
  const unsigned obs_block_bad = wave_bad[0][0] | wave_bad[0][1] | wave_bad[0][2] | wave_bad[0][3];
  for (int t = 0; t < T; ++t) cell_o[t][tid] = rd_iss_cell(words[0][1 + t], cy, cx);
  if (L == 6 && wave == 0)
    for (int t = 0; t < T; ++t) {
      unsigned n = (unsigned)__popcll(words[0][1 + t][lane]);
#pragma unroll
      for (int k = 1; k < 64; k <<= 1) n += __shfl_xor(n, k);
      if (lane == 0) so6[t] = n;
    }
  __syncthreads();                                                            // (buffer 0 is the second member's)

  // lanes of a tile: 4^(L - 2) for L = 2 .. 5; the leader counts the tile
  const int group = L >= 6 ? 64 : (L >= 2 ? 1 << (2 * (L - 2)) : 1);
  const bool leader = L >= 6 ? tid == 0 : (lane & (group - 1)) == 0;
  const int top = L < 5 ? L : 5;                                              // the last level the waves count for themselves
  unsigned n_valid = 0, n_void = 0;

  for (int m = ma; m < mb; ++m) {
    const int buf = (m - ma + 1) & 1;
    pack(v, buf);
    if (m + 1 < mb) load(members + (long)(m + 1) * member_stride, v);
    __syncthreads();
    // the void rule: the bits of this cell that lie in a valid tile
    const unsigned bad16 = (rd_iss_cell(words[buf][0], cy, cx) | bad_o16) & in16;
    unsigned ok16;
    bool block_bad = false;
    if (L == 1) {
      ok16 = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned mk = (0x33u << (2 * (k & 1))) << (8 * (k >> 1));
        const bool in = (in16 & mk) != 0, bad = (bad16 & mk) != 0;
        ok16 |= in && !bad ? mk : 0u;
        n_valid += in && !bad;
        n_void += in && bad;
      }
    } else {
      unsigned bad = bad16 != 0;
      if (L >= 6) {
        bad = obs_block_bad | wave_bad[buf][0] | wave_bad[buf][1] | wave_bad[buf][2] | wave_bad[buf][3];
        block_bad = bad != 0;
      } else {
        for (int k = 1; k < group; k <<= 1) bad |= __shfl_xor(bad, k);
      }
      ok16 = bad ? 0u : in16;
      if (L <= 6 && leader && in16) {
        n_valid += !bad;
        n_void += bad != 0;
      }
    }
    const int slot = (int)((long)(m - m0) * gridDim.y + blockIdx.y);          // the pair of a pass (L > 6)
    if (L > 6 && tid == 0) held_flags[(long)slot * gridDim.x + blockIdx.x] = block_bad;

    for (int t = 0; t < T; ++t) {
      const unsigned x16 = rd_iss_cell(words[buf][1 + t], cy, cx) & ok16, o16 = cell_o[t][tid] & ok16;
      // levels 0 and 2: the cell's counts; level 1: its four 2 x 2 blocks
      const unsigned sx2 = __popc(x16), so2 = __popc(o16);
      unsigned q1x = 0, q1o = 0, q1xo = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned mk = (0x33u << (2 * (k & 1))) << (8 * (k >> 1));
        const unsigned a = __popc(x16 & mk), c = __popc(o16 & mk);
        q1x += a * a, q1o += c * c, q1xo += a * c;
      }
      unsigned long long px = sx2 | ((unsigned long long)q1x << 12) | ((unsigned long long)(sx2 * sx2) << 26);
      unsigned long long po = so2 | ((unsigned long long)q1o << 12) | ((unsigned long long)(so2 * so2) << 26);
      unsigned long long pxo = __popc(x16 & o16) | ((unsigned long long)q1xo << 12) | ((unsigned long long)(sx2 * so2) << 26);
      // level 3: 4 lanes
      unsigned s = sx2 | (so2 << 16);
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      if ((lane & 3) == 0) {
        const unsigned long long a = s & 0xFFFFu, c = s >> 16;
        px |= (a * a) << 42, po |= (c * c) << 42, pxo |= (a * c) << 42;
      }
      // level 4: 16 lanes
      s += __shfl_xor(s, 4);
      s += __shfl_xor(s, 8);
      unsigned long long p4 = 0;
      if ((lane & 15) == 0) {
        const unsigned long long a = s & 0xFFFFu, c = s >> 16;
        p4 = (a * a) | ((c * c) << 20) | ((a * c) << 40);
      }
      // level 5: the wave
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      p4 += rd_iss_shfl_xor64(p4, 16);
      p4 += rd_iss_shfl_xor64(p4, 32);
#pragma unroll
      for (int k = 1; k < 64; k <<= 1) {
        px += rd_iss_shfl_xor64(px, k);
        po += rd_iss_shfl_xor64(po, k);
        pxo += rd_iss_shfl_xor64(pxo, k);
      }
      if (lane == 0) {
        const unsigned long long a5 = s & 0xFFFFu, c5 = s >> 16;
        unsigned long long q[6][3];
        const unsigned long long p[3] = {px, po, pxo};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          q[0][k] = p[k] & 0xFFFull, q[1][k] = (p[k] >> 12) & 0x3FFFull, q[2][k] = (p[k] >> 26) & 0xFFFFull, q[3][k] = (p[k] >> 42) & 0x3FFFFull;
          q[4][k] = (p4 >> (20 * k)) & 0xFFFFFull;
        }
        q[5][0] = a5 * a5, q[5][1] = c5 * c5, q[5][2] = a5 * c5;
        if (L <= 6) {
#pragma unroll
          for (int l = 0; l < 6; ++l)
            if (l <= top)
#pragma unroll
              for (int k = 0; k < 3; ++k)
                if (q[l][k]) atomicAdd(&cnt[t][l][k], q[l][k]);
        } else {
          unsigned* rec = held + ((((long)slot * gridDim.x + blockIdx.x) * T + t) * 4 + wave) * RD_ISS_REC;
#pragma unroll
          for (int l = 0; l < 6; ++l)
#pragma unroll
            for (int k = 0; k < 3; ++k) rec[l * 3 + k] = (unsigned)q[l][k];
          rec[18] = (unsigned)a5, rec[19] = (unsigned)c5;
        }
      }
      if (L == 6 && wave == 0) {                                              // the block is the tile: a lane per row word
        unsigned n = block_bad ? 0u : (unsigned)__popcll(words[buf][1 + t][lane]);
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) n += __shfl_xor(n, k);
        if (lane == 0 && !block_bad) {
          const unsigned long long a = n, c = so6[t];
          if (a) atomicAdd(&cnt[t][6][0], a * a);
          if (c) atomicAdd(&cnt[t][6][1], c * c);
          if (a && c) atomicAdd(&cnt[t][6][2], a * c);
        }
      }
    }
  }
  if (L > 6) return;
  // the tiles this workgroup counted, and its counters
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    n_valid += __shfl_xor(n_valid, k);
    n_void += __shfl_xor(n_void, k);
  }
  if (lane == 0) {
    if (n_valid) atomicAdd(&tile_cnt[0], n_valid);
    if (n_void) atomicAdd(&tile_cnt[1], n_void);
  }
  __syncthreads();
  if (tid < 2 && tile_cnt[tid]) atomicAdd(&tiles[hour * 2 + tid], (unsigned long long)tile_cnt[tid]);
  const int per_t = (L + 1) * 3;
  for (int i = tid; i < T * per_t; i += RD_ISS_THREADS) {
    const int t = i / per_t, r = i % per_t;
    const unsigned long long c = cnt[t][r / 3][r % 3];
    if (c) atomicAdd(&counts[((long)t * RD_HOURS + hour) * per_t + r], c);
  }
}

// L = 7 .. 10.  grid (tiles of a plane, units of the pass, members of the pass); one workgroup per (pair, tile).  Thread i < 4^(L - 6)
// takes the block whose Morton code inside the tile is i
__global__ void __launch_bounds__(RD_ISS_THREADS)
k_iss_upper(const unsigned* __restrict__ held, const unsigned* __restrict__ held_flags, rd_iss_geo g, int T, long u0,
            unsigned long long* __restrict__ counts, unsigned long long* __restrict__ tiles) {
  __shared__ unsigned sx[2][RD_ISS_THREADS], so[2][RD_ISS_THREADS];
  __shared__ unsigned long long cnt[RD_ISS_MAXL + 1][3];
  const int tid = threadIdx.x, L = g.L, up = L - 6, nblk = 1 << (2 * up);      // blocks of a tile: 4 .. 256
  const int hour = (int)((u0 + blockIdx.y) % RD_HOURS);
  const int tiles_x = g.cx >> L, ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x % tiles_x;
  const long slot = (long)blockIdx.z * gridDim.y + blockIdx.y, nblocks = (long)g.nby * g.nbx;
  long blk = 0;
  int bad = 0;
  if (tid < nblk) {
    int bx = 0, by = 0;
    for (int k = 0; k < up; ++k) bx |= ((tid >> (2 * k)) & 1) << k, by |= ((tid >> (2 * k + 1)) & 1) << k;
    blk = (long)((ty << up) + by) * g.nbx + (tx << up) + bx;
    bad = held_flags[slot * nblocks + blk] != 0;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicAdd(&tiles[hour * 2 + 1], 1ull);
    return;
  }
  if (tid == 0) atomicAdd(&tiles[hour * 2], 1ull);
  const int per_t = (L + 1) * 3;
  for (int t = 0; t < T; ++t) {
    for (int i = tid; i < per_t; i += RD_ISS_THREADS) (&cnt[0][0])[i] = 0ull;
    __syncthreads();
    if (tid < nblk) {
      const unsigned* rec = held + ((slot * nblocks + blk) * T + t) * 4 * RD_ISS_REC;
      unsigned long long q[6][3];
      unsigned a = 0, c = 0;
#pragma unroll
      for (int i = 0; i < 18; ++i) q[i / 3][i % 3] = 0ull;
      for (int w = 0; w < 4; ++w) {
#pragma unroll
        for (int i = 0; i < 18; ++i) q[i / 3][i % 3] += rec[w * RD_ISS_REC + i];
        a += rec[w * RD_ISS_REC + 18], c += rec[w * RD_ISS_REC + 19];
      }
#pragma unroll
      for (int i = 0; i < 18; ++i)
        if (q[i / 3][i % 3]) atomicAdd(&cnt[i / 3][i % 3], q[i / 3][i % 3]);
      if (a) atomicAdd(&cnt[6][0], (unsigned long long)a * a);
      if (c) atomicAdd(&cnt[6][1], (unsigned long long)c * c);
      if (a && c) atomicAdd(&cnt[6][2], (unsigned long long)a * c);
      sx[0][tid] = a, so[0][tid] = c;
    }
    __syncthreads();
    for (int l = 7, n = nblk >> 2, src = 0; l <= L; ++l, n >>= 2, src ^= 1) {  // level l: n blocks, each four of level l - 1
      if (tid < n) {
        const unsigned a = sx[src][4 * tid] + sx[src][4 * tid + 1] + sx[src][4 * tid + 2] + sx[src][4 * tid + 3];
        const unsigned c = so[src][4 * tid] + so[src][4 * tid + 1] + so[src][4 * tid + 2] + so[src][4 * tid + 3];
        sx[src ^ 1][tid] = a, so[src ^ 1][tid] = c;
        if (a) atomicAdd(&cnt[l][0], (unsigned long long)a * a);
        if (c) atomicAdd(&cnt[l][1], (unsigned long long)c * c);
        if (a && c) atomicAdd(&cnt[l][2], (unsigned long long)a * c);
      }
      __syncthreads();
    }
    for (int i = tid; i < per_t; i += RD_ISS_THREADS) {
      const unsigned long long c = (&cnt[0][0])[i];
      if (c) atomicAdd(&counts[((long)t * RD_HOURS + hour) * per_t + i], c);
    }
    __syncthreads();
  }
}
