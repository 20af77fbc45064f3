// The body of drop_add_ln_bwd_kernel and drop_add_ln_bwd_kernel_det (csrc/ln.hip), textually included INSIDE both kernel
// functions: not a standalone header (a shared __device__ function changed the default kernel's code).  In scope where it is
// included: NCH, the constant DET and the kernel's parameters.
  __shared__ float s_g[4][256 * NCH], s_b[4][256 * NCH];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int grp = blockIdx.y, Mg = a.M / a.groups;
  if constexpr (DET) dgb += (long)blockIdx.x * gridDim.y * 2 * a.H;
  if (grp) { gamma = a.gamma2; dgb += 2 * a.H; }
  const unsigned seed = ln_seed(a);
  float ag[4 * NCH], ab[4 * NCH], gm[4 * NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const float4 g = *reinterpret_cast<const float4 *>(gamma + ch * 256 + lane * 4);
    gm[ch * 4 + 0] = g.x; gm[ch * 4 + 1] = g.y; gm[ch * 4 + 2] = g.z; gm[ch * 4 + 3] = g.w;
  }
#pragma unroll
  for (int i = 0; i < 4 * NCH; ++i) { ag[i] = 0.0f; ab[i] = 0.0f; }
  const float invH = 1.0f / (float)a.H;
  // the loads of row r + stride are issued BEFORE row r is reduced (a wave otherwise has one row = 6 KB in flight and
  // waits a full memory round trip per row: 2.5 TB/s at the ViT shape)
  struct Raw {
    bf16x4 x[NCH], r[NCH], d[NCH], s[NCH];
    float mean, rstd;
  };
  const bf16x4 zero4 = {(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
  auto fetch = [&](int row, Raw &w) {
    const long rowoff = (long)row * a.H;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = ch * 256 + lane * 4;
      w.x[ch] = *reinterpret_cast<const bf16x4 *>(x + rowoff + c0);
      w.r[ch] = res ? *reinterpret_cast<const bf16x4 *>(res + rowoff + c0) : zero4;
      w.d[ch] = *reinterpret_cast<const bf16x4 *>(dy + rowoff + c0);
      w.s[ch] = dsum ? *reinterpret_cast<const bf16x4 *>(dsum + rowoff + c0) : zero4;
    }
    w.mean = mean_in[row];
    w.rstd = rstd_in[row];
  };
  const int row_end = (grp + 1) * Mg, stride = gridDim.x * 4;
  int row = grp * Mg + blockIdx.x * 4 + wid;
  Raw cur, nxt;
  if (row < row_end) fetch(row, cur);
  for (; row < row_end; row += stride) {
    const bool more = row + stride < row_end;  // wave-uniform
    if (more) fetch(row + stride, nxt);
    const long rowoff = (long)row * a.H;
    float z[4 * NCH], g[4 * NCH];
    const float ps = ln_path_scale(a, seed, row);
    const float mean = cur.mean, rstd = cur.rstd;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = ch * 256 + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = ch * 4 + j;
        float v = (float)cur.x[ch][j];
        if (a.thresh) v = ln_keep(seed, row, c0 + j, a.thresh) ? v * a.inv_keep : 0.0f;
        z[i] = a.x_is_sum ? v : v * ps + (float)cur.r[ch][j];   // dropout(x) * path + residual, as load_z (or the stored sum)
        const float dyv = (float)cur.d[ch][j];
        z[i] = (z[i] - mean) * rstd;  // z_hat
        g[i] = dyv * gm[i];
        s1 += g[i];
        s2 += g[i] * z[i];
        ag[i] += dyv * z[i];
        ab[i] += dyv;
      }
    }
    s1 = wave_sum_f32(s1) * invH;
    s2 = wave_sum_f32(s2) * invH;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = ch * 256 + lane * 4;
      bf16x4 ox, orr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = ch * 4 + j;
        const float dz = rstd * (g[i] - s1 - z[i] * s2) + (float)cur.s[ch][j];
        orr[j] = (__bf16)dz;
        float dxv = dz * ps;
        if (a.thresh) dxv = ln_keep(seed, row, c0 + j, a.thresh) ? dxv * a.inv_keep : 0.0f;
        ox[j] = (__bf16)dxv;
      }
      *reinterpret_cast<bf16x4 *>(dx + rowoff + c0) = ox;
      if (dres) *reinterpret_cast<bf16x4 *>(dres + rowoff + c0) = orr;
    }
    if (more) cur = nxt;
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s_g[wid][ch * 256 + lane * 4 + j] = ag[ch * 4 + j];
      s_b[wid][ch * 256 + lane * 4 + j] = ab[ch * 4 + j];
    }
  __syncthreads();
  constexpr int H = 256 * NCH;
  for (int c = threadIdx.x; c < H; c += 256) {
    if constexpr (DET) {
      dgb[c] = (s_g[0][c] + s_g[1][c]) + (s_g[2][c] + s_g[3][c]);
      dgb[H + c] = (s_b[0][c] + s_b[1][c]) + (s_b[2][c] + s_b[3][c]);
    } else {
      atomicAdd(dgb + c, (s_g[0][c] + s_g[1][c]) + (s_g[2][c] + s_g[3][c]));
      atomicAdd(dgb + H + c, (s_b[0][c] + s_b[1][c]) + (s_b[2][c] + s_b[3][c]));
    }
  }

