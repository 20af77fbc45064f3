// The body of gemm64_kernel and gemm64_kernel_det (csrc/gemm.hip), textually included INSIDE both kernel functions: not a
// standalone header.  One text, two kernels, and the default kernel's code is exactly what it was before the deterministic
// variant existed (a shared __device__ function changed its register allocation and LDS layout).  In scope where it is
// included: the template parameters BJ, P_XC, Q_XC, EPI, OUT_F32, KT, NS, the constant DET and the kernel argument `args`.
  static_assert(BJ == 64 || (BJ == 32 && !Q_XC), "32-wide j tiles only for K-contiguous Q");
  static_assert(KT == 1 || KT == 2 || (KT == 4 && BJ == 32), "one, two or (32-row tiles) four K tiles per step");
  constexpr int QF = BJ / 32;               // 16-wide j fragments per wave
  constexpr int Q_UNIT = BJ * 128;          // bytes of the Q image per K tile
  constexpr int TILE_BYTES = 8192 + Q_UNIT;
  constexpr int STAGE = KT * TILE_BYTES;
  // NS LDS stages, NS - 1 K tiles in flight.  MEASURED (profiles/r02_gemm_bench_v2.json): 5 stages instead of 3 change
  // nothing for the forward / dX forms (a K tile costs ~0.24 us either way: the loop is bound by the ISSUE of its 3-4
  // LDS-DMA instructions per wave, ~100 cycles each, not by memory latency) and halve the weight-gradient form
  // (80 KB of LDS = 2 workgroups per CU for a kernel that lives on its output stores) => 3.
  static_assert(NS >= 3 && NS * STAGE <= 160 * 1024, "LDS stages");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  const int t = blockIdx.x;
  int pi = 0;
  for (int k = 1; k < args.n; ++k)
    if (t >= args.p[k].tile0) pi = k;
  const GemmProblem &pr = args.p[pi];
  const int ksplit = OUT_F32 ? pr.ksplit() : 1;
  const int Ni = pr.Ni, Nj = pr.Nj, Kc = pr.Kc;
  int tl = t - pr.tile0, ks = 0;
  if (ksplit > 1) {
    // a cut contraction (detector weight gradients: millions of rows, 1 - 8 output tiles): the output tiles of ONE piece
    // read the same rows of both operands, so they get neighbouring slots of the same XCD (workgroups go to the XCDs
    // round-robin by blockIdx) and meet in its L2 (PMC: operands fetched once) -- 170 -> 125 us on SA2's first layer
    // against the piece-major order that spreads them over the XCDs
    const int lt = t - pr.tile0;
    const int ntl = pr.tiles_i() * ((Nj + BJ - 1) / BJ);
    if ((ksplit & 7) == 0 && (pr.tile0 & 7) == 0) {
      const int slot = lt >> 3;
      tl = slot % ntl;
      ks = (slot / ntl) * 8 + (lt & 7);
    } else {
      tl = lt % ntl;
      ks = lt / ntl;
    }
  }
  const int bj = tl / pr.tiles_i(), bi = tl % pr.tiles_i();
  const int i0 = bi * 64, j0 = bj * BJ;
  const int ldp = pr.ldp, ldq = pr.ldq;
  const int nkt_all = (Kc + 63) >> 6;
  const int kt_per = (nkt_all + ksplit - 1) / ksplit;
  const int kt0 = ks * kt_per;                         // this workgroup's K tiles: [kt0, kt0 + nkt)
  const int nkt = max(0, min(kt_per, nkt_all - kt0));

  const auto rsP = __builtin_amdgcn_make_buffer_rsrc((void *)pr.P, 0, pr.p_bytes, 0x00020000);
  const auto rsQ = __builtin_amdgcn_make_buffer_rsrc((void *)pr.Q, 0, pr.q_bytes, 0x00020000);
  const int cp = lane & 7;
  // P unit: 2 DMAs per wave (rows (2w+d)*8 + lane/8); Q unit: 2 (BJ = 64) or 1 (BJ = 32: rows w*8 + lane/8)
  unsigned vp[2], vq[2];
  // XC Q under a row map (short contractions over a strided (batch, rows) view): the contraction row each DMA stages next
  // and its column offset.  SCALARS on purpose: as small arrays hipcc promoted them to LDS (+ 4 KB per workgroup) and every
  // gemm64 launch of the step got 10-20 us slower (profiles/r04: 15.2 -> 27.1 us on the text side's dX form)
  const bool q_xc_map = Q_XC && pr.q_rpb() != 0;   // (workgroup-uniform)
  int qrow0 = 0, qrow1 = 0;
  unsigned qcol0 = 0, qcol1 = 0;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const int ur = (wave * 2 + d) * 8 + (lane >> 3);
    if (!P_XC) vp[d] = (unsigned)(((i0 + ur) * ldp + (cp ^ (ur & 7)) * 8) * 2);
    else vp[d] = (unsigned)((ur * ldp + i0 + (cp ^ (xg(ur) << 1)) * 8) * 2);
    const int uq = (BJ == 64) ? ur : wave * 8 + (lane >> 3);
    // (batched-row map of Q, GemmProblem::q_rpb: on its j rows here, on its contraction rows in the XC form -- see stage())
    if (!Q_XC) vq[d] = (mapped_row(j0 + uq, ldq, pr.q_rpb(), pr.q_bstride) + (unsigned)((cp ^ (uq & 7)) * 8)) * 2u;
    else vq[d] = (unsigned)((uq * ldq + j0 + (cp ^ (xg(uq) << 1)) * 8) * 2);
    if (Q_XC) {
      const int row = kt0 * 64 + uq;
      const unsigned col = (unsigned)(j0 + (cp ^ (xg(uq) << 1)) * 8);
      if (d == 0) { qrow0 = row; qcol0 = col; } else { qrow1 = row; qcol1 = col; }
    }
  }
  const unsigned p_step = P_XC ? (unsigned)(64 * ldp * 2) : 128u;
  const unsigned q_step = Q_XC ? (unsigned)(64 * ldq * 2) : 128u;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    vp[d] += (unsigned)kt0 * p_step;
    vq[d] += (unsigned)kt0 * q_step;
  }
  constexpr int NDMA = KT * (2 + (BJ == 64 ? 2 : 1));  // LDS-DMAs per wave per step

  auto stage = [&](int step) {
#pragma unroll
    for (int h = 0; h < KT; ++h) {
      const bool live = step * KT + h < nkt;
      const unsigned base = (unsigned)((step % NS) * STAGE + h * TILE_BYTES);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsP, (lds_void_t *)(smem + base + (wave * 2 + d) * 1024), 16,
                                                 live ? vp[d] : 0x80000000u, 0, 0, 0);
        vp[d] += p_step;
      }
#pragma unroll
      for (int d = 0; d < (BJ == 64 ? 2 : 1); ++d) {
        const int blk = (BJ == 64) ? wave * 2 + d : wave;
        if (Q_XC && q_xc_map) {   // short contractions over a strided (batch, rows) view: one division per DMA
          if (d == 0) { vq[0] = (mapped_row(qrow0, ldq, pr.q_rpb(), pr.q_bstride) + qcol0) * 2u; qrow0 += 64; }
          else { vq[1] = (mapped_row(qrow1, ldq, pr.q_rpb(), pr.q_bstride) + qcol1) * 2u; qrow1 += 64; }
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (lds_void_t *)(smem + base + 8192 + blk * 1024), 16,
                                                 live ? vq[d] : 0x80000000u, 0, 0, 0);
        vq[d] += q_step;
      }
    }
  };

  const int row16 = lane & 15, q4 = lane >> 4;
  const int kc_base = row16 * 128 + ((q4 ^ (row16 & 7)) << 4);
  // (XC fragment addresses in closed form: read_frag_cf, gemm_common.h -- sub16 depends on the wave here)
  const int xc_q = (lane & 15) >> 2, xcg = (xc_q >> 1) | ((q4 & 1) << 1);
  const int xc0 = (8 * q4 + xc_q) * 128 + 8 * (lane & 3);

  f32x4 acc[2][QF];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < QF; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // weight-gradient form with pr.colsum set: the column sums of Q over this workgroup's share of the contraction (the
  // bias gradient) from all-ones MFMAs on the B fragments, waves wr == 0 of the i = 0 tiles (see gemm256_kernel)
  constexpr bool QSUM = P_XC && Q_XC && OUT_F32;
  const bool do_qsum = QSUM && pr.colsum != nullptr && bi == 0 && wr == 0;   // wave-uniform
  f32x4 qs[QF];
  bf16x8 ones;
#pragma unroll
  for (int b = 0; b < QF; ++b) qs[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

#pragma unroll
  for (int p = 0; p < NS - 1; ++p) stage(p);
  const int nsteps = (nkt + KT - 1) / KT;
  for (int step = 0; step < nsteps; ++step) {
    // step `step` has landed for this wave (steps step+1 .. step+NS-2 may still be in flight); after the barrier: for
    // every wave, and every wave has finished reading the buffer that step step+NS-1 is about to overwrite
    static_assert((NS - 2) * NDMA <= 63, "vmcnt is a 6-bit counter");
    wait_vmcnt<(NS - 2) * NDMA>();
    BQ_BARRIER();
    stage(step + NS - 1);
#pragma unroll
    for (int h = 0; h < KT; ++h) {  // (a K tile past the end was staged as zeros: it adds nothing)
      const unsigned char *buf = smem + (step % NS) * STAGE + h * TILE_BYTES;
      bf16x8 fa[2][2], fb[QF][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) fa[a][kk] = read_frag_cf_x<P_XC>(buf, wr * 2 + a, kk, kc_base, xc0, xcg);
#pragma unroll
      for (int b = 0; b < QF; ++b)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) fb[b][kk] = read_frag_cf_x<Q_XC>(buf + 8192, wc * QF + b, kk, kc_base, xc0, xcg);
      if (P_XC || Q_XC) {
        // (round 6) the contraction-major reads are inline asm: behind stage() hipcc fenced them with vmcnt(0) -- every step
        // of the weight-gradient forms waited for the DMAs it had just issued for step + NS - 1 (tools/isa_waits.py)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < QF; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a][kk], fb[b][kk], acc[a][b], 0, 0, 0);
      if (QSUM && do_qsum) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int b = 0; b < QF; ++b) qs[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, fb[b][kk], qs[b], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: straight from the accumulators (8-B bf16 / 16-B fp32 pieces of an output row) ---------------------
  const int ldo = pr.ldo;
  const int iw = i0 + wr * 32, jw = j0 + wc * (BJ / 2);
  const bool atomic_out = ksplit > 1 || pr.accum();   // fp32 out: add to what is there (cut contraction / second row source)
  if (QSUM && do_qsum && q4 == 0) {
#pragma unroll
    for (int b = 0; b < QF; ++b) {
      const int j = jw + b * 16 + row16;
      if (j < Nj) {
        if (!atomic_out) pr.colsum[j] = qs[b][0];
        else if constexpr (DET) pr.colsum[j] = pr.colsum[j] + qs[b][0];   // (accum only: the host refuses ksplit > 1 with colsum)
        else atomicAdd(pr.colsum + j, qs[b][0]);   // (zero-initialised by the caller, as `out` is)
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int i = iw + a * 16 + q4 * 4;
    float b4[4] = {0.f, 0.f, 0.f, 0.f};
    if ((EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) && pr.bias != nullptr && i < Ni) load_bias4(pr, i, b4);
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < QF; ++b) {
      const int j = jw + b * 16 + row16;
      const bool ok = j < Nj && i < Ni;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[a][b][r] + b4[r];
      // element offset of row j of out / out2 / aux (64-bit on plain rows: outputs beyond 2 G elements exist)
      const long jo = pr.o_rpb() ? (long)mapped_row(j < Nj ? j : 0, ldo, pr.o_rpb(), pr.o_bstride) : (long)j * ldo;
      if (OUT_F32) {
        float *dst = reinterpret_cast<float *>(pr.out) + jo + i;
        if constexpr (DET) {
          if (ksplit > 1) dst += (long)ks * Nj * ldo;   // this piece's slab (no row map: host check)
          if (ok && pr.accum()) {
            const float4 o = *reinterpret_cast<const float4 *>(dst);
            *reinterpret_cast<float4 *>(dst) = make_float4(o.x + v[0], o.y + v[1], o.z + v[2], o.w + v[3]);
          } else if (ok) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
          }
          continue;
        }
        if (ok && !atomic_out) *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        if (ok && atomic_out) {
#pragma unroll
          for (int r = 0; r < 4; ++r) atomicAdd(dst + r, v[r]);
        }
        continue;
      }
      if (EPI == EPI_DGELU && ok) {
        const bf16x4 y = *reinterpret_cast<const bf16x4 *>(pr.aux + jo + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= dgelu_f((float)y[r]);
      }
      if (EPI == EPI_ADD && ok) {
        const bf16x4 y = *reinterpret_cast<const bf16x4 *>(pr.aux + jo + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)y[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (float)(__bf16)v[r];
      if (ok) {
        uint2 pk;
        pk.x = pack_bf16x2(v[0], v[1]);
        pk.y = pack_bf16x2(v[2], v[3]);
        *reinterpret_cast<uint2 *>(reinterpret_cast<__bf16 *>(pr.out) + jo + i) = pk;
        if (EPI == EPI_BIAS_GELU) {
          pk.x = pack_bf16x2(gelu_f(v[0]), gelu_f(v[1]));
          pk.y = pack_bf16x2(gelu_f(v[2]), gelu_f(v[3]));
          *reinterpret_cast<uint2 *>(reinterpret_cast<__bf16 *>(pr.out2) + jo + i) = pk;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) cs[r] += ok ? v[r] : 0.f;
    }
    if (!OUT_F32 && pr.colsum != nullptr) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = cs[r];
        s += dpp_f32_add<0x111>(s);
        s += dpp_f32_add<0x112>(s);
        s += dpp_f32_add<0x114>(s);
        s += dpp_f32_add<0x118>(s);
        if (row16 == 15 && i + r < Ni) atomicAdd(pr.colsum + i + r, s);
      }
    }
  }
