// The body of colsum_grouped_kernel and colsum_grouped_det_kernel (csrc/gemm.hip), textually included INSIDE both kernel
// functions: not a standalone header (see gemm64_kernel_body.h).  In scope: the constant DET, `args` and `partial`.
  __shared__ float red[8][256];
  const int t = blockIdx.x;
  int pi = 0;
  for (int k = 1; k < args.n; ++k)
    if (t >= args.p[k].wg0) pi = k;
  const ColsumProblem &pr = args.p[pi];
  const int tl = t - pr.wg0;
  const int cb = tl % pr.cblocks, rb = tl / pr.cblocks;
  const int tc = threadIdx.x & 31, tr = threadIdx.x >> 5;
  const int col = cb * 256 + tc * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (col < pr.N) {  // N % 8 == 0
    const int r1 = min(pr.M, (rb + 1) * COLSUM_ROWS);
    for (int r = rb * COLSUM_ROWS + tr; r < r1; r += 8) {
      const bf16x8 v = *reinterpret_cast<const bf16x8 *>(pr.g + (long)r * pr.ld + col);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tr][tc * 8 + e] = s[e];
  __syncthreads();
  const int c = threadIdx.x;
  float tot = 0.f;
#pragma unroll
  for (int g8 = 0; g8 < 8; ++g8) tot += red[g8][c];
  if constexpr (DET) partial[(long)t * 256 + c] = tot;
  else if (cb * 256 + c < pr.N) atomicAdd(pr.out + cb * 256 + c, tot);

