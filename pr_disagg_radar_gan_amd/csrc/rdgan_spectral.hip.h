// Log-spectral distance (reference log_spectral_distance.py): radial power spectra of (nd, nd) fields and the distance of every
// pair of them, reduced on the device to a histogram and moments.
#pragma once

#define RD_SPEC_MAXND 64
#define RD_SPEC_MAXK 48
#define RD_LSD_TILE 128
#define RD_LSD_MAXROWS (1L << 22)          // rows of A or B: keeps a workgroup's LDS bin counts (<= 128 M) below 2^32
#define RD_LSD_MAX_DYN_LDS (57344L)        // 64 KiB less the 8 KiB of static reduction arrays of k_lsd_pairwise

// Radial bin of shifted pixel (i, j) about the centre ((nd - 1) / 2, (nd - 1) / 2): with p = 2 j - (nd - 1), q = 2 i - (nd - 1)
// (both odd) the radius is sqrt(p^2 + q^2) / 2 and bin = floor(radius) = the largest b with 4 b^2 <= p^2 + q^2.  p^2 + q^2 is 2
// mod 4, so no pixel sits on an integer radius: the bin is exact in integers; the float sqrt only seeds the search.
__host__ __device__ inline int rd_spec_bin(int p, int q) {
  const int s = p * p + q * q;
  int b = (int)(sqrtf((float)s) * 0.5f);
  while (4 * (b + 1) * (b + 1) <= s) ++b;
  while (4 * b * b > s) --b;
  return b;
}

// host-made tables, passed by value in the kernel-argument segment
struct rd_spec_args {
  float tw_re[RD_SPEC_MAXND], tw_im[RD_SPEC_MAXND];   // exp(-2 pi i j / nd), computed in double and rounded once
  int cnt[RD_SPEC_MAXK];                              // pixels in kept bin 1 + b
};

// One workgroup per field (four per workgroup at nd 8).  Row DFT then column DFT through LDS, one output frequency per thread
// and pass; |F|^2 by unshifted frequency; a deterministic per-bin sum (each shifted row walks its pixels in order into its own
// partial row, then one thread per bin adds the rows in order); mean over the bin, optionally 10 log10.
// Frequencies k != 0 are summed over x[n] - x[0] (the same value in exact arithmetic): a constant row or column then gives
// exactly 0 there, as the reference's FFT does, instead of the rounding residue of the twiddle table -- a dry or constant field
// must come out with P_k = 0 in every kept bin, because that decides NaN versus a finite distance.
template <int ND>
__global__ __launch_bounds__(256) void k_radial_spectra(const float* __restrict__ x, float* __restrict__ out, int N, int K,
                                                        int logout, rd_spec_args a) {
  constexpr int NN = ND * ND;
  constexpr int FPB = NN >= 256 ? 1 : 256 / NN;
  __shared__ __attribute__((aligned(16))) float xs[FPB * NN];   // fields; after the row pass the power |F|^2
  __shared__ __attribute__((aligned(16))) float2 rs[FPB * NN];  // row DFT; after the column pass the per-row bin partials
  __shared__ float2 tw[ND];
  float* part = (float*)rs;                                      // [FPB][ND][K], K < 2 ND
  const int t = threadIdx.x;
  const long f0 = (long)blockIdx.x * FPB;
  for (int i = t; i < ND; i += 256) tw[i] = make_float2(a.tw_re[i], a.tw_im[i]);
  for (int i = t; i < FPB * NN / 4; i += 256) {
    const long f = f0 + (4 * i) / NN;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f < N) v = *(const float4*)(x + f0 * NN + 4L * i);
    *(float4*)(xs + 4 * i) = v;
  }
  __syncthreads();
  // row pass: R[y][k] = sum_n (x[y][n] - (k ? x[y][0] : 0)) w^(k n)
  for (int o = t; o < FPB * NN; o += 256) {
    const int k = o % ND;
    const float* row = xs + (o - k);
    const float x0 = k ? row[0] : 0.f;
    float re = 0.f, im = 0.f;
    int idx = 0;
#pragma unroll
    for (int n = 0; n < ND; n += 4) {
      const float4 v4 = *(const float4*)(row + n);
      const float v[4] = {v4.x - x0, v4.y - x0, v4.z - x0, v4.w - x0};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float2 w = tw[idx];
        re = fmaf(v[u], w.x, re);
        im = fmaf(v[u], w.y, im);
        idx += k;
        if (idx >= ND) idx -= ND;
      }
    }
    rs[o] = make_float2(re, im);
  }
  __syncthreads();
  // column pass: F[l][k] = sum_y (R[y][k] - (l ? R[0][k] : 0)) w^(l y);  P = |F|^2 into xs
  for (int o = t; o < FPB * NN; o += 256) {
    const int fl = o / NN, r = o % NN, l = r / ND, k = r % ND;
    const float2* col = rs + fl * NN + k;
    const float2 c0 = l ? col[0] : make_float2(0.f, 0.f);
    float re = 0.f, im = 0.f;
    int idx = 0;
#pragma unroll
    for (int y = 0; y < ND; ++y) {
      const float2 v = col[y * ND];
      const float vr = v.x - c0.x, vi = v.y - c0.y;
      const float2 w = tw[idx];
      re = fmaf(vr, w.x, fmaf(-vi, w.y, re));
      im = fmaf(vr, w.y, fmaf(vi, w.x, im));
      idx += l;
      if (idx >= ND) idx -= ND;
    }
    xs[o] = re * re + im * im;
  }
  __syncthreads();
  for (int i = t; i < FPB * ND * K; i += 256) part[i] = 0.f;
  __syncthreads();
  // per shifted row i: walk the shifted columns j in order, one run per bin (a row meets a bin in at most two runs)
  for (int w = t; w < FPB * ND; w += 256) {
    const int fl = w / ND, i = w % ND;
    const float* P = xs + fl * NN + ((i + ND / 2) % ND) * ND;   // fftshift: shifted index i is frequency (i + nd/2) mod nd
    float* prt = part + w * K;
    const int q = 2 * i - (ND - 1);
    int cur = -1;
    float acc = 0.f;
    for (int j = 0; j < ND; ++j) {
      const int b = rd_spec_bin(2 * j - (ND - 1), q);
      if (b != cur) {
        if (cur >= 1 && cur <= K) prt[cur - 1] += acc;
        acc = 0.f;
        cur = b;
      }
      acc += P[(j + ND / 2) % ND];
    }
    if (cur >= 1 && cur <= K) prt[cur - 1] += acc;
  }
  __syncthreads();
  for (int w = t; w < FPB * K; w += 256) {
    const int fl = w / K, b = w % K;
    const long f = f0 + fl;
    if (f >= N) continue;
    float s = 0.f;
    for (int i = 0; i < ND; ++i) s += part[(fl * ND + i) * K + b];
    const float mean = s / (float)a.cnt[b];
    out[f * K + b] = logout ? 10.f * log10f(mean) : mean;
  }
}

// Per-workgroup moments of the finite distances (fp64 sums), reduced in a fixed order by k_lsd_reduce.
struct rd_lsd_partial {
  double sum, sq;
  long long cnt;
  float mn, mx;
};

// Pairwise LSD of log-spectra A [N][K] and B [M][K] (dB): d(i, j) = sqrt(sum_k (A[i][k] - B[j][k])^2) * (1 / K), in the
// difference form (no |a|^2 + |b|^2 - 2 a.b: the dB values reach tens and the cancellation would swamp small distances).
// Workgroup = a 128-row strip of A against the column tiles blockIdx.x, blockIdx.x + gridDim.x, ...; 256 threads, 8 x 8 pairs
// each (rows 4 ty + r and 64 + 4 ty + r, columns alike with tx), both operands K-major in LDS.
// Outputs (each optional): dist [N][M] (16-byte stores where the row allows); hist [nbins + 4] (uint64: bins, then below lo,
// at or above hi, NaN, +inf), counted per workgroup with LDS integer atomics and added once per workgroup and bin with 64-bit
// vector atomics (integer: order-free, so bit-identical); part [gridDim.x * gridDim.y] moments for k_lsd_reduce.
// Bin rule (fp32): b = (int)floorf((d - lo) * scale), scale = (float)nbins / (hi - lo), b clamped to nbins - 1.
// excl_diag: the pairs i == j are left out of hist and moments and written as 0 in dist (the reference never writes them).
__global__ __launch_bounds__(256) void k_lsd_pairwise(const float* __restrict__ A, const float* __restrict__ B, int N, int M,
                                                      int K, int excl_diag, float* __restrict__ dist,
                                                      unsigned long long* __restrict__ hist, int nbins, float lo, float hi,
                                                      float scale, rd_lsd_partial* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lsd_sm[];
  float* As = lsd_sm;                                  // [K][128]
  float* Bs = lsd_sm + K * RD_LSD_TILE;                // [K][128]
  unsigned* h = (unsigned*)(Bs + K * RD_LSD_TILE);     // [nbins + 4] when hist
  __shared__ double r_sum[256], r_sq[256];
  __shared__ long long r_cnt[256];
  __shared__ float r_mn[256], r_mx[256];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int i0 = blockIdx.y * RD_LSD_TILE;
  const int ntj = (M + RD_LSD_TILE - 1) / RD_LSD_TILE;
  const float invK = 1.f / (float)K;
  if (hist)
    for (int b = t; b < nbins + 4; b += 256) h[b] = 0u;
  for (int e = t; e < RD_LSD_TILE * K; e += 256) {
    const int r = e / K, k = e % K, i = i0 + r;
    As[k * RD_LSD_TILE + r] = i < N ? A[(long)i * K + k] : 0.f;
  }
  long long cnt = 0;
  double sum = 0.0, sq = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int jt = blockIdx.x; jt < ntj; jt += gridDim.x) {
    const int j0 = jt * RD_LSD_TILE;
    __syncthreads();                                   // previous tile's Bs reads are done
    for (int e = t; e < RD_LSD_TILE * K; e += 256) {
      const int c = e / K, k = e % K, j = j0 + c;
      Bs[k * RD_LSD_TILE + c] = j < M ? B[(long)j * K + k] : 0.f;
    }
    __syncthreads();
    float acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float4 a0 = *(const float4*)(As + k * RD_LSD_TILE + 4 * ty), a1 = *(const float4*)(As + k * RD_LSD_TILE + 64 + 4 * ty);
      const float4 b0 = *(const float4*)(Bs + k * RD_LSD_TILE + 4 * tx), b1 = *(const float4*)(Bs + k * RD_LSD_TILE + 64 + 4 * tx);
      const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float d = av[r] - bv[c];
          acc[r][c] = fmaf(d, d, acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = i0 + (r < 4 ? 4 * ty + r : 64 + 4 * ty + r - 4);
      if (i >= N) continue;
#pragma unroll
      for (int hc = 0; hc < 2; ++hc) {
        const int jb = j0 + 64 * hc + 4 * tx;
        float dv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = jb + c;
          const float d = sqrtf(acc[r][4 * hc + c]) * invK;
          const bool use = j < M && !(excl_diag && i == j);
          dv[c] = use ? d : 0.f;
          if (!use) continue;
          if (hist || part) {
            if (d != d) {
              if (hist) atomicAdd(&h[nbins + 2], 1u);
            } else if (d == INFINITY) {
              if (hist) atomicAdd(&h[nbins + 3], 1u);
            } else {
              ++cnt;
              sum += (double)d;
              sq += (double)d * (double)d;
              mn = fminf(mn, d);
              mx = fmaxf(mx, d);
              if (hist) {
                int b;
                if (d < lo) b = nbins;
                else if (d >= hi) b = nbins + 1;
                else b = min((int)floorf((d - lo) * scale), nbins - 1);
                atomicAdd(&h[b], 1u);
              }
            }
          }
        }
        if (dist) {
          float* row = dist + (long)i * M;
          if ((M & 3) == 0 && jb + 3 < M) {
            *(float4*)(row + jb) = make_float4(dv[0], dv[1], dv[2], dv[3]);
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (jb + c < M) row[jb + c] = dv[c];
          }
        }
      }
    }
  }
  __syncthreads();
  if (hist)
    for (int b = t; b < nbins + 4; b += 256) {
      const unsigned v = h[b];
      if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
  if (!part) return;
  r_sum[t] = sum; r_sq[t] = sq; r_cnt[t] = cnt; r_mn[t] = mn; r_mx[t] = mx;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      r_sum[t] += r_sum[t + s]; r_sq[t] += r_sq[t + s]; r_cnt[t] += r_cnt[t + s];
      r_mn[t] = fminf(r_mn[t], r_mn[t + s]); r_mx[t] = fmaxf(r_mx[t], r_mx[t + s]);
    }
  }
  if (t == 0) {
    rd_lsd_partial p;
    p.sum = r_sum[0]; p.sq = r_sq[0]; p.cnt = r_cnt[0]; p.mn = r_mn[0]; p.mx = r_mx[0];
    part[blockIdx.y * gridDim.x + blockIdx.x] = p;
  }
}

// One workgroup: the partials in a fixed order (thread t takes t, t + 256, ..., then a fixed tree), so repeated calls agree bit
// for bit.  out[5] = count, sum, sum of squares, min, max of the finite distances.
__global__ __launch_bounds__(256) void k_lsd_reduce(const rd_lsd_partial* __restrict__ part, int nparts, double* __restrict__ out) {
  __shared__ double r_sum[256], r_sq[256];
  __shared__ long long r_cnt[256];
  __shared__ float r_mn[256], r_mx[256];
  const int t = threadIdx.x;
  double sum = 0.0, sq = 0.0;
  long long cnt = 0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = t; i < nparts; i += 256) {
    const rd_lsd_partial p = part[i];
    sum += p.sum; sq += p.sq; cnt += p.cnt;
    mn = fminf(mn, p.mn); mx = fmaxf(mx, p.mx);
  }
  r_sum[t] = sum; r_sq[t] = sq; r_cnt[t] = cnt; r_mn[t] = mn; r_mx[t] = mx;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
      r_sum[t] += r_sum[t + s]; r_sq[t] += r_sq[t + s]; r_cnt[t] += r_cnt[t + s];
      r_mn[t] = fminf(r_mn[t], r_mn[t + s]); r_mx[t] = fmaxf(r_mx[t], r_mx[t + s]);
    }
  }
  if (t == 0) {
    out[0] = (double)r_cnt[0]; out[1] = r_sum[0]; out[2] = r_sq[0]; out[3] = r_mn[0]; out[4] = r_mx[0];
  }
}
