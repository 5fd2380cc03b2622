// Chaining scenarios across midnight: how well every member of one day continues every member of the next,
// the cheapest single series through the days, and a greedy matching of the members of neighbouring days.
// Everything is an integer.  A value x of an hourly array is good when 0 <= x < 2048 (rd_depth_bad); a good value has the feature
// e = min(rint(x * 32), 65535), a uint16 in units of 1/32 mm, rint to even; a bad value has the feature 0 and sets the bad bit of
// its (day, edge, pixel).  A day has two edges: edge 0 is its first_hour, edge 1 its last_hour.  Boundary b joins edge 1 of day b
// to edge 0 of day b + shift; pixel p is masked there when either bad bit is set; n_valid[b] counts the others.
// C[b][i][j] = sum over the unmasked p of |e(day b, member i, edge 1, p) - e(day b + shift, member j, edge 0, p)| < 2^16 2^24 = 2^40,
// and key = C << 24 | i << 12 | j orders the pairs of a boundary strictly (i, j < 4096).
//
// Layouts.  P = ny nx pixels, padded to Ppad = 8 ceil(P / 8); a uint4 holds 8 pixels, U = Ppad / 8; padding pixels are 0 on both
// sides and never bad.
//  * features [member][day][edge][Ppad] uint16; bad [day][edge][W] 32-bit words, W = ceil(Ppad / 32), bit p % 32 of word p / 32.
//  * costs [B][S_a][S_b] int64, B = n_days - shift; back [B][S] int32; perm [B][S] int32.
// Kernels.
//  * k_seq_edges<VEC>: one thread per (unit, edge, 8 pixels) reads the two chosen hours only, writes the features and ORs the bad
//    bits into the words of day unit % n_days.
//  * k_seq_valid: n_valid[b] = P - popcount(bad_a | bad_b), a fixed tree.
//  * k_seq_costs: a workgroup of 256 threads owns a 64 x 64 tile of pairs of one boundary and a range of pixel chunks.  A chunk is
//    128 pixels: the 64 row members' and the 64 column members' 16 uint4 are staged in LDS as [uint4 of the chunk][member] (row
//    stride 65 uint4, so the 16 stores of consecutive lanes fall on different banks), a masked pixel zeroed on both sides while it
//    is staged, the next chunk fetched to registers while the current one is used.  A thread keeps rows ty + 16 r and columns
//    tx + 16 k (r, k = 0 .. 3): 16 32-bit sums, one v_sad_u16 per two pixels of a pair, and adds them to 16 64-bit sums every
//    RD_SEQ_FLUSH chunks.  The sums of a tile's pixel ranges meet in the zeroed output through 64-bit integer atomics: exact in
//    any order.
//  * k_seq_minplus: one step acc'[j] = min over i of acc[i] + C[i][j] with the smallest such i in back[j].
//  * k_seq_match_init / _minima / _take: a round of the locally dominant matching.  minima: a workgroup owns 8 rows and walks the
//    free columns once: the row minima of its free rows go to rowmin, the minima of its rows per column into colmin by a 64-bit
//    atomic minimum.  take: row i is matched to the column j of rowmin[i] iff colmin[j] is the same key; the free flags, perm and
//    the count of free rows follow, and the colmin of the next round is emptied.  With a count of 0 both return at once.
// Kernel boundaries are the only ordering: no spin-wait, no grid sync, no workgroup waits for another.  All global offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "rdgan_hourly.hip.h"

#define RD_SEQ_MAXS 4096                 // members: i and j take 12 bits each of a key
#define RD_SEQ_UNIT 32                   // features are integers in 1 / RD_SEQ_UNIT mm
#define RD_SEQ_FEATMAX 65535
#define RD_SEQ_MAXDAYS 65535             // days of an ensemble: the boundaries of a matching are the grid's y
#define RD_SEQ_MAXCOSTS (1L << 31)       // elements of one call's cost array
#define RD_SEQ_THREADS 256
#define RD_SEQ_TILE 64                   // rows and columns of a tile of pairs
#define RD_SEQ_CHUNK 16                  // uint4 of a member in a chunk: 128 pixels
#define RD_SEQ_LDU 65                    // uint4 of an LDS row: RD_SEQ_TILE members and one of padding
// chunks between two additions to the 64-bit sums: 256 * 128 = 32768 pixels, and 32768 * 65535 < 2^31 < 2^32 (65536 pixels would
// still fit: 65536 * 65535 = 2^32 - 65536)
#define RD_SEQ_FLUSH 256
#define RD_SEQ_TARGET_BLOCKS 2048        // workgroups a costs launch aims at: eight per compute unit
#define RD_SEQ_ROWS 8                    // rows of a workgroup of k_seq_match_minima
#define RD_SEQ_COLS (RD_SEQ_MAXS / RD_SEQ_THREADS)   // columns of a thread there
#define RD_SEQ_EMPTY (~0ull)

static_assert((long)RD_SEQ_FLUSH * RD_SEQ_CHUNK * 8 * RD_SEQ_FEATMAX < (1L << 32), "the 32-bit sums of a pair must not wrap");
static_assert(RD_SEQ_MAXS == 1 << 12 && RD_HOURLY_MAXPLANE * (RD_SEQ_FEATMAX + 1L) <= 1L << 40, "key = cost << 24 | i << 12 | j");

__host__ __device__ inline long rd_seq_ppad(long plane) { return (plane + 7) / 8 * 8; }
__host__ __device__ inline long rd_seq_words(long plane) { return (rd_seq_ppad(plane) + 31) / 32; }
__host__ __device__ inline long rd_seq_tiles(long s) { return (s + RD_SEQ_TILE - 1) / RD_SEQ_TILE; }
// the workspace of one boundary's matching, bytes: rowmin [S], colmin [2][S] 64-bit, then the free flags of rows and columns
__host__ __device__ inline long rd_seq_match_bytes(long s) { return (26 * s + 7) / 8 * 8; }

__device__ __forceinline__ unsigned rd_seq_feature(float v) {
  return min((unsigned)rintf(v * (float)RD_SEQ_UNIT), (unsigned)RD_SEQ_FEATMAX);
}

// grid (ceil(n 2 U / 256)); item = (unit * 2 + edge) * U + c.  VEC needs x 16-byte aligned and plane and day_stride multiples of 4.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_seq_edges(const float* __restrict__ x, long n, long day_stride, int plane, int U, int W, long n_days, int first_hour, int last_hour,
            uint4* __restrict__ feat, unsigned* __restrict__ bad) {
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= n * 2 * U) return;
  const long ue = item / U, unit = ue >> 1;
  const int c = (int)(item - ue * U), edge = (int)(ue & 1), p0 = c * 8;
  const float* xp = x + unit * day_stride + (long)(edge ? last_hour : first_hour) * plane + p0;
  float v[8];
  if constexpr (VEC) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (p0 < plane) a = *reinterpret_cast<const float4*>(xp);
    if (p0 + 4 < plane) b = *reinterpret_cast<const float4*>(xp + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p0 + i < plane ? xp[i] : 0.0f;
  }
  unsigned e[8], bits = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool b = rd_depth_bad(v[i]);
    e[i] = b ? 0u : rd_seq_feature(v[i]);
    bits |= b ? 1u << i : 0u;
  }
  feat[item] = make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16);
  if (bits) atomicOr(&bad[((unit % n_days) * 2 + edge) * W + (c >> 2)], bits << ((c & 3) * 8));
}

// grid (B): n_valid[b] = plane - the masked pixels of boundary b
__global__ void __launch_bounds__(256)
k_seq_valid(const unsigned* __restrict__ bad_a, const unsigned* __restrict__ bad_b, int W, int shift, long plane, long long* __restrict__ n_valid) {
  __shared__ unsigned part[4];
  const long b = blockIdx.x;
  const unsigned* wa = bad_a + (b * 2 + 1) * W;
  const unsigned* wb = bad_b + ((b + shift) * 2) * W;
  unsigned count = 0u;
  for (int w = threadIdx.x; w < W; w += 256) count += __popc(wa[w] | wb[w]);
  for (int s = 32; s > 0; s >>= 1) count += __shfl_xor(count, s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) n_valid[b] = plane - (long long)(part[0] + part[1] + part[2] + part[3]);
}

// 0xFFFF for each of the two pixels 2k, 2k + 1 of a uint4 whose bit of `bits` is clear
__device__ __forceinline__ unsigned rd_seq_keep2(unsigned bits, int k) {
  const unsigned t = ((bits >> (2 * k)) & 1u) | (((bits >> (2 * k + 1)) & 1u) << 16);
  return ~(t * 0xFFFFu);
}

// what a thread stages of a chunk: the same uint4 of four members of the row side and of four of the column side, and the bad
// bits of its 8 pixels
struct rd_seq_stage {
  uint4 a[4], b[4];
  unsigned bits;
};

// grid (B * TA * TB * nsplit): split fastest, then the column tile, the row tile, the boundary.  fa, fb: the features of the row
// and the column ensemble; member strides in uint4.  costs is zeroed before the launch.
__global__ void __launch_bounds__(RD_SEQ_THREADS)
k_seq_costs(const uint4* __restrict__ fa, const unsigned* __restrict__ bad_a, int Sa, const uint4* __restrict__ fb,
            const unsigned* __restrict__ bad_b, int Sb, long n_days, int U, int W, int shift, int TA, int TB, int nsplit, int chunks_per_split,
            unsigned long long* __restrict__ costs) {
  __shared__ __attribute__((aligned(16))) uint4 rows[RD_SEQ_CHUNK * RD_SEQ_LDU], cols[RD_SEQ_CHUNK * RD_SEQ_LDU];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  long idx = blockIdx.x;
  const int sp = (int)(idx % nsplit); idx /= nsplit;
  const int tj = (int)(idx % TB); idx /= TB;
  const int ti = (int)(idx % TA);
  const long b = idx / TA;
  const int nchunks = (U + RD_SEQ_CHUNK - 1) / RD_SEQ_CHUNK;
  const int c0 = sp * chunks_per_split, c1 = min(c0 + chunks_per_split, nchunks);
  if (c0 >= c1) return;                                                    // (uniform)
  const long stride = n_days * 2 * U;                                      // uint4 of a member
  const uint4* pa = fa + (b * 2 + 1) * U;                                  // edge 1 of day b
  const uint4* pb = fb + ((b + shift) * 2) * U;                            // edge 0 of day b + shift
  const unsigned* wa = bad_a + (b * 2 + 1) * W;
  const unsigned* wb = bad_b + ((b + shift) * 2) * W;
  // the staging slots of this thread: q = 0 .. 3, slot = tid + 256 q: member slot / 16 of the tile, uint4 slot % 16 of the chunk
  const int su = tid & (RD_SEQ_CHUNK - 1), sm = tid >> 4;                  // (sm + 16 q: the member)
  rd_seq_stage st;
  auto fetch = [&](int c) {
    const int u = c * RD_SEQ_CHUNK + su;
    const bool in = u < U;
    const unsigned w = in ? (wa[u >> 2] | wb[u >> 2]) : 0u;
    st.bits = (w >> ((u & 3) * 8)) & 0xFFu;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ma = ti * RD_SEQ_TILE + sm + 16 * q, mb = tj * RD_SEQ_TILE + sm + 16 * q;
      st.a[q] = in && ma < Sa ? pa[ma * stride + u] : make_uint4(0u, 0u, 0u, 0u);
      st.b[q] = in && mb < Sb ? pb[mb * stride + u] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  unsigned acc[4][4];
  unsigned long long tot[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = 0u, tot[r][k] = 0ull;
  fetch(c0);
  for (int c = c0; c < c1; ++c) {
    __syncthreads();                                                       // the previous chunk has been used
    {
      const unsigned k0 = rd_seq_keep2(st.bits, 0), k1 = rd_seq_keep2(st.bits, 1), k2 = rd_seq_keep2(st.bits, 2), k3 = rd_seq_keep2(st.bits, 3);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int at = su * RD_SEQ_LDU + sm + 16 * q;
        rows[at] = make_uint4(st.a[q].x & k0, st.a[q].y & k1, st.a[q].z & k2, st.a[q].w & k3);
        cols[at] = make_uint4(st.b[q].x & k0, st.b[q].y & k1, st.b[q].z & k2, st.b[q].w & k3);
      }
    }
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);
#pragma unroll 4
    for (int u = 0; u < RD_SEQ_CHUNK; ++u) {
      uint4 e[4], f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = rows[u * RD_SEQ_LDU + ty + 16 * r];
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = cols[u * RD_SEQ_LDU + tx + 16 * k];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          unsigned a = acc[r][k];
          a = __builtin_amdgcn_sad_u16(e[r].x, f[k].x, a);
          a = __builtin_amdgcn_sad_u16(e[r].y, f[k].y, a);
          a = __builtin_amdgcn_sad_u16(e[r].z, f[k].z, a);
          a = __builtin_amdgcn_sad_u16(e[r].w, f[k].w, a);
          acc[r][k] = a;
        }
    }
    if ((c - c0) % RD_SEQ_FLUSH == RD_SEQ_FLUSH - 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[r][k] += acc[r][k], acc[r][k] = 0u;
    }
  }
  unsigned long long* out = costs + b * Sa * Sb;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = ti * RD_SEQ_TILE + ty + 16 * r, j = tj * RD_SEQ_TILE + tx + 16 * k;
      const unsigned long long v = tot[r][k] + acc[r][k];
      if (i < Sa && j < Sb && v) atomicAdd(&out[(long)i * Sb + j], v);
    }
}

// grid (ceil(S / 64)): thread (column tid % 64, slice tid / 64) walks the rows slice, slice + 4, ...; the slices meet in LDS
__global__ void __launch_bounds__(256)
k_seq_minplus(const long long* __restrict__ C, int S, const long long* __restrict__ acc, long long* __restrict__ acc_next, int* __restrict__ back) {
  __shared__ long long sv[4][64];
  __shared__ int si[4][64];
  const int jl = threadIdx.x & 63, slice = threadIdx.x >> 6, j = blockIdx.x * 64 + jl;
  long long best = 0x7FFFFFFFFFFFFFFFll;
  int bi = 0x7FFFFFFF;
  if (j < S)
    for (int i = slice; i < S; i += 4) {
      const long long v = acc[i] + C[(long)i * S + j];
      if (v < best) best = v, bi = i;                                      // (ascending i: the first of equals stays)
    }
  sv[slice][jl] = best, si[slice][jl] = bi;
  __syncthreads();
  if (slice == 0 && j < S) {
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      const long long v = sv[s][jl];
      const int i = si[s][jl];
      if (v < best || (v == best && i < bi)) best = v, bi = i;
    }
    acc_next[j] = best, back[j] = bi;
  }
}

// the matching state of boundary b inside the workspace
struct rd_seq_match_state {
  unsigned long long *rowmin, *colmin0, *colmin1;
  unsigned char *row_free, *col_free;
};
__device__ __forceinline__ rd_seq_match_state rd_seq_state(void* workspace, long b, int S) {
  unsigned char* base = (unsigned char*)workspace + b * rd_seq_match_bytes(S);
  rd_seq_match_state s;
  s.rowmin = (unsigned long long*)base, s.colmin0 = s.rowmin + S, s.colmin1 = s.colmin0 + S;
  s.row_free = base + 24l * S, s.col_free = s.row_free + S;
  return s;
}

// grid (ceil(S / 256), B).  full: a new matching -- every row and column free, perm -1; otherwise only the column minima are emptied
__global__ void __launch_bounds__(256)
k_seq_match_init(int S, int full, int* __restrict__ perm, int* __restrict__ free_rows, void* __restrict__ workspace) {
  const long b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const rd_seq_match_state s = rd_seq_state(workspace, b, S);
  if (i >= S) return;
  s.colmin0[i] = RD_SEQ_EMPTY, s.colmin1[i] = RD_SEQ_EMPTY;
  if (full) {
    s.rowmin[i] = RD_SEQ_EMPTY, s.row_free[i] = 1, s.col_free[i] = 1, perm[b * S + i] = -1;
    if (i == 0) free_rows[b] = S;
  }
}

// grid (ceil(S / 8), B): the minima of the keys of 8 rows over the free columns, per row and per column
__global__ void __launch_bounds__(RD_SEQ_THREADS)
k_seq_match_minima(const long long* __restrict__ costs, int S, int parity, const int* __restrict__ free_rows, void* __restrict__ workspace) {
  __shared__ unsigned long long part[RD_SEQ_THREADS / 64][RD_SEQ_ROWS];
  const long b = blockIdx.y;
  if (free_rows[b] == 0) return;                                           // (uniform: the matching is complete)
  const int tid = threadIdx.x, i0 = blockIdx.x * RD_SEQ_ROWS;
  const rd_seq_match_state s = rd_seq_state(workspace, b, S);
  unsigned long long* colmin = parity ? s.colmin1 : s.colmin0;
  const long long* C = costs + b * S * S;
  unsigned cf = 0u;
#pragma unroll
  for (int k = 0; k < RD_SEQ_COLS; ++k) {
    const int j = tid + RD_SEQ_THREADS * k;
    if (j < S && s.col_free[j]) cf |= 1u << k;
  }
  unsigned long long rmin[RD_SEQ_ROWS], cmin[RD_SEQ_COLS];
#pragma unroll
  for (int r = 0; r < RD_SEQ_ROWS; ++r) rmin[r] = RD_SEQ_EMPTY;
#pragma unroll
  for (int k = 0; k < RD_SEQ_COLS; ++k) cmin[k] = RD_SEQ_EMPTY;
#pragma unroll
  for (int r = 0; r < RD_SEQ_ROWS; ++r) {
    const int i = i0 + r;
    if (i < S && s.row_free[i]) {                                          // (uniform)
#pragma unroll
      for (int k = 0; k < RD_SEQ_COLS; ++k) {
        const int j = tid + RD_SEQ_THREADS * k;
        if (cf >> k & 1u) {
          const unsigned long long key = ((unsigned long long)C[(long)i * S + j] << 24) | ((unsigned long long)i << 12) | (unsigned long long)j;
          rmin[r] = key < rmin[r] ? key : rmin[r];
          cmin[k] = key < cmin[k] ? key : cmin[k];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RD_SEQ_ROWS; ++r) {
    unsigned long long v = rmin[r];
    for (int sft = 32; sft > 0; sft >>= 1) {
      const unsigned long long o = __shfl_xor(v, sft);
      v = o < v ? o : v;
    }
    if ((tid & 63) == 0) part[tid >> 6][r] = v;
  }
  __syncthreads();
  if (tid < RD_SEQ_ROWS && i0 + tid < S && s.row_free[i0 + tid]) {
    unsigned long long v = part[0][tid];
#pragma unroll
    for (int w = 1; w < RD_SEQ_THREADS / 64; ++w) v = part[w][tid] < v ? part[w][tid] : v;
    s.rowmin[i0 + tid] = v;
  }
#pragma unroll
  for (int k = 0; k < RD_SEQ_COLS; ++k)
    if (cmin[k] != RD_SEQ_EMPTY) atomicMin(&colmin[tid + RD_SEQ_THREADS * k], cmin[k]);
}

// grid (ceil(S / 256), B): the locally dominant pairs are taken; the column minima of the next round are emptied
__global__ void __launch_bounds__(256)
k_seq_match_take(int S, int parity, int* __restrict__ perm, int* __restrict__ free_rows, void* __restrict__ workspace) {
  const long b = blockIdx.y;
  // (a count of 0 seen here means every pair has been written: a workgroup lowers the count after its own pairs)
  if (free_rows[b] == 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const rd_seq_match_state s = rd_seq_state(workspace, b, S);
  const unsigned long long* colmin = parity ? s.colmin1 : s.colmin0;
  unsigned long long* colnext = parity ? s.colmin0 : s.colmin1;
  bool taken = false;
  if (i < S) {
    colnext[i] = RD_SEQ_EMPTY;
    if (s.row_free[i]) {
      const unsigned long long key = s.rowmin[i];
      const int j = (int)(key & 0xFFFull);
      if (key != RD_SEQ_EMPTY && j < S && colmin[j] == key) {
        perm[b * S + i] = j;
        s.row_free[i] = 0, s.col_free[j] = 0;
        taken = true;
      }
    }
  }
  const unsigned long long m = __ballot(taken);
  if ((threadIdx.x & 63) == 0 && m) atomicSub(&free_rows[b], (int)__popcll(m));
}
