// l12fwd_body.h -- the BODY of k_l12fwd and k_l12fwd_pf (l1fused.hip), included inside both kernels.  In scope at the point of
// inclusion: the template parameters ACT, NT2, TWIN, NTS, ROW1, the constant PFZ, and the kernel arguments a, a2 (L12Args).
// Text, not a __device__ function: called through a (force-inlined) function, hipcc optimises the body before it knows that the
// argument pointers are global ones and schedules the layer-2 K loop of the EARLIER forms differently -- it opens the second block of
// every pair with s_waitcnt vmcnt(0), half the prefetch depth.  Included as text, the kernels that existed before PFZ keep their code.
// No include guard: it is meant to be included more than once.
  if (TWIN && blockIdx.y) a = a2;
  constexpr int NW = 8, NT = 2, H1 = L12_H1, NTHREADS = 512, N2 = NW * NT2 * 32;
  constexpr int PFX = 2;                                      // 16-k blocks of layer-2 weight fragments in flight
  static_assert(!PFZ || (ROW1 && NT2 == 1), "PFZ is a form of the ROW1 kernel for hidden[1] = 256");
  static_assert(!PFZ || PFX * NT2 * X_NP == NT * X_NP, "PFZ: the K loop's fragment slots hold exactly one 16-k block of the first-layer image");
  // h1 image: rows of 2 * 512 bytes PADDED by 16 (stride 260 dwords: the 16 rows of a ds_read_b128 service group start 4 banks
  // apart -- conflict free without an XOR swizzle, so every store / fragment address is one per-lane base + a compile-time
  // offset; the swizzled form cost ~4 VALU and a live register per element and made hipcc spill 200 registers)
  constexpr int AROW = L12_AROW, APLANE = LF_ROWS * AROW;
  extern __shared__ __attribute__((aligned(16))) char l12_smem[];
  char* Aimg = l12_smem;                                      // 2 planes [32][512 k]
  char* Xs0 = Aimg + X_NP * APLANE;                           // 2 buffers x 2 planes [32][32 k] of observations
  float* redA = reinterpret_cast<float*>(Xs0 + 2 * X_NP * LF_XPLANE);   // [2][NW][32]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
  const bool lb0 = (lane & 1) != 0, lb1 = (lane & 2) != 0;
  float* totA = redA + 2 * NW * 32 + w * 64;                  // this wave's folded [2][32]
  const int O = a.O;
  const float xs = a.xmax ? x_scale_from_max(*a.xmax, X_ASCALE) : X_ASCALE;
  const float xinv = 1.0f / xs;
  constexpr int w1_step = (H1 / 32) * X_NP * 64;              // u32x4 entries per 16-k block of the W1 image
  // PFZ: the K loop's fragment slots live across tiles -- between two K loops they hold block 0 of the first-layer image (slot u:
  // column tile u) -- and four more quads hold its block 1 from the end of a K loop to the next tile's z1 product
  u32x4 bxo[PFZ ? PFX : 1][NT2][X_NP];
  u32x4 w1r[PFZ ? NT : 1][X_NP];
  if constexpr (PFZ) {                // the first tile's eight fragments, in front of the parameter and observation loads
    const u32x4* __restrict__ w1q = reinterpret_cast<const u32x4*>(a.W1x) + (int64_t)(w * NT) * X_NP * 64 + lane;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int p = 0; p < X_NP; ++p) {
        bxo[j][0][p] = w1q[(j * X_NP + p) * 64];
        w1r[j][p] = w1q[w1_step + (j * X_NP + p) * 64];
      }
  }
  float bias[NT], gam[NT], bet[NT], b2v[NT2];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = w * 32 * NT + 32 * j + li;
    bias[j] = a.b1[col];
    gam[j] = a.g[col];
    bet[j] = a.be[col];
  }
#pragma unroll
  for (int j = 0; j < NT2; ++j) b2v[j] = a.b2[w * 32 * NT2 + 32 * j + li];
  const u32x4* __restrict__ W1x = reinterpret_cast<const u32x4*>(a.W1x) + (int64_t)(w * NT) * X_NP * 64 + lane;
  typedef const u32x4 __attribute__((address_space(1))) * gfrag_t;
  // PFZ: this wave's first-layer image behind a pointer hipcc cannot see through (still in the global address space: global loads,
  // counted waits) -- the eight fragment addresses are formed where they are used, from one register pair, not hoisted and spilled
  auto w1_image = [&]() -> gfrag_t {
    const u32x4* q = W1x;
    asm volatile("" : "+v"(q));
    return (gfrag_t)q;
  };
  const u32x4* __restrict__ W2x = reinterpret_cast<const u32x4*>(a.W2x) + (int64_t)(w * NT2) * X_NP * 64 + lane;
  constexpr int w2_step = (N2 / 32) * X_NP * 64;
  const float invH = 1.0f / (float)H1;
  const int64_t ntiles = (a.M + LF_ROWS - 1) / LF_ROWS;
  constexpr int XN = LF_ROWS * 32 / NTHREADS;                 // 2 observation values per thread and tile
  float xr[XN];
  auto t_opaque = [&]() -> int {      // PFZ: see the kernels' head comment (l1fused.hip)
    int tt = t;
    if (PFZ) asm volatile("" : "+v"(tt));
    return tt;
  };
  auto x_load = [&](int64_t tl) {
    const int ts = t_opaque();
#pragma unroll
    for (int c = 0; c < XN; ++c) {
      const int i = ts + c * NTHREADS, r = i >> 5, k = i & 31;
      if constexpr (PFZ) {
        const bool ok = k < O && tl * LF_ROWS + r < a.M;
        const float v = a.X[ok ? (tl * LF_ROWS + r) * O + k : (int64_t)0];      // always issued: the counted waits behind it hold on every path
        xr[c] = ok ? v : 0.f;
      } else {
        xr[c] = (k < O && tl * LF_ROWS + r < a.M) ? a.X[(tl * LF_ROWS + r) * O + k] : 0.f;
      }
    }
  };
  auto x_store = [&](int b) {
    char* Xd = Xs0 + b * X_NP * LF_XPLANE;
    const int ts = t_opaque();
#pragma unroll
    for (int c = 0; c < XN; ++c) {
      const int i = ts + c * NTHREADS;
      l12_xa_stage(Xd, i >> 5, i & 31, xr[c], xs);
    }
  };
  if ((int64_t)blockIdx.x < ntiles) {
    x_load(blockIdx.x);
    x_store(0);
  }
  int buf = 0;
  // phase stamps (tools/l12_phases.py): compiled in only with -DRLX_L12_STAMPS=1 -- the counter costs the kernel three spilled registers
#if RLX_L12_STAMPS
  int sti = 0;
#define L12_STAMP() if (a.stamps && t == 0 && blockIdx.x == 0 && blockIdx.y == 0 && sti < 14) a.stamps[sti++] = clock64();
#define L12_WALL(I) if (a.stamps && t == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.stamps[I] = wall_clock64();      // constant 100 MHz: calibrates the clock64 ticks
#else
#define L12_STAMP()
#define L12_WALL(I)
#endif
  L12_STAMP()
  L12_WALL(14)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    const int64_t r0 = tile * LF_ROWS;
    const bool has_next = tile + gridDim.x < ntiles;
    __syncthreads();      // this tile's observation planes are visible; the previous tile's readers of the h1 image are done
    L12_STAMP()
    u32x4 bxi[PFZ ? 1 : PFX][NT2][X_NP];
    auto& bx = [&]() -> auto& { if constexpr (PFZ) return bxo; else return bxi; }();      // the K loop's fragment slots
    if (PFZ || has_next) x_load(tile + gridDim.x);      // PFZ: always, branch-free, and behind every fragment request of this tile's z1
    // ---- z1 = X @ W1 + b1 on the fp16 pipe (the recompute of k_dx_l1bwd)
    f32x16 z[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      float zb = bias[j] * (xs * X_WSCALE);
      // (PFZ: formed per tile.  Hoisted out of the tile loop -- the earlier form -- the two splat accumulator images pin 32 registers for
      //  the whole kernel, which is what makes hipcc spill the staging pointers)
      if (PFZ) asm volatile("" : "+v"(zb));
#pragma unroll
      for (int r = 0; r < 16; ++r) z[j][r] = zb;
    }
    {
      const char* xa = Xs0 + buf * X_NP * LF_XPLANE;
      const int nks = O > 16 ? 2 : 1;
      if constexpr (PFZ) {
        // both blocks' weight fragments are in registers (bx: the K loop's wrapped refills, w1r: requested behind it; first tile: the
        // prologue): no loads here; with O <= 16 the second block (all zero words) was fetched and is not multiplied
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
          u32x4 xf[X_NP];
#pragma unroll
          for (int p = 0; p < X_NP; ++p) xf[p] = *reinterpret_cast<const u32x4*>(xa + p * LF_XPLANE + bx_off(li, 2 * s_ + lh));
          if (s_ < nks) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              const u32x4 w0 = s_ ? w1r[j][0] : bx[j][0][0], w1 = s_ ? w1r[j][1] : bx[j][0][1];
              z[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xf[0]), __builtin_bit_cast(f16x8, w1), z[j], 0, 0, 0);
              z[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xf[1]), __builtin_bit_cast(f16x8, w0), z[j], 0, 0, 0);
              z[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xf[0]), __builtin_bit_cast(f16x8, w0), z[j], 0, 0, 0);
            }
          }
        }
      } else {
      const u32x4* w1l = W1x;
      asm volatile("" : "+v"(w1l));      // re-load the 8 fragments per tile (L1 / L2 hits): hoisted out of the tile loop they pin 32 registers
      // (behind the asm the pointer is GENERIC to the compiler: it emitted flat_load_dwordx4 + s_waitcnt vmcnt(0) lgkmcnt(0) per
      //  fragment pair -- four serial L2 round trips per tile.  Back to the global address space: global loads with counted waits for
      //  the first 16-k block -- one exposed L2 round trip.  The second block, O > 16, reuses one register quad and still goes load,
      //  s_waitcnt vmcnt(0), MFMA three times over: three more serial round trips.  The PFZ form above has none of them.)
      gfrag_t w1p = (gfrag_t)w1l;
      for (int s_ = 0; s_ < nks; ++s_) {
        u32x4 xf[X_NP];
#pragma unroll
        for (int p = 0; p < X_NP; ++p) xf[p] = *reinterpret_cast<const u32x4*>(xa + p * LF_XPLANE + bx_off(li, 2 * s_ + lh));
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const u32x4 w0 = w1p[(int64_t)s_ * w1_step + (j * X_NP + 0) * 64], w1 = w1p[(int64_t)s_ * w1_step + (j * X_NP + 1) * 64];
          z[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xf[0]), __builtin_bit_cast(f16x8, w1), z[j], 0, 0, 0);
          z[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xf[1]), __builtin_bit_cast(f16x8, w0), z[j], 0, 0, 0);
          z[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xf[0]), __builtin_bit_cast(f16x8, w0), z[j], 0, 0, 0);
        }
      }
      }
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[j][r] *= xinv * X_WINV;
    }
    if (!PFZ && has_next) x_store(buf ^ 1);       // (its last readers finished before this tile's first barrier; PFZ: behind the K loop)
    L12_STAMP()
    // ---- LayerNorm row statistics (as k_l1fwd_mfma / k_dx_l1bwd)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float sv[4], ssv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * gq + e;
        float s_ = 0.f, ss = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) { s_ += z[j][r]; ss += z[j][r] * z[j][r]; }
        sv[e] = s_;
        ssv[e] = ss;
      }
      const float st_ = half_sum4(sv[0], sv[1], sv[2], sv[3], lb0, lb1);
      const float sst = half_sum4(ssv[0], ssv[1], ssv[2], ssv[3], lb0, lb1);
      if (li < 4) {
        redA[(0 * NW + w) * 32 + 8 * gq + 4 * lh + li] = st_;
        redA[(1 * NW + w) * 32 + 8 * gq + 4 * lh + li] = sst;
      }
    }
    __syncthreads();
    {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < NW; ++q) v += redA[((lane >> 5) * NW + q) * 32 + (lane & 31)];
      float rs_row;
      totA[lane] = ROW1 ? ln_row_stats(v, lane, invH, rs_row) : v;      // ROW1: mean | 1 / std in the sums' place
    }
    if (a.stats && w == 0 && lane < 32 && r0 + lane < a.M) {      // [2][M]: what the recomputing weight-gradient kernel reads
      if (ROW1) {
        a.stats[r0 + lane] = totA[lane];
        a.stats[a.M + r0 + lane] = totA[32 + lane];
      } else {
        const float mean = totA[lane] * invH;
        a.stats[r0 + lane] = mean;
        a.stats[a.M + r0 + lane] = rsqrtf(fmaxf(0.f, totA[32 + lane] * invH - mean * mean) + 1e-6f);
      }
    }
    L12_STAMP()
    // ---- normalise, activate; h1 -> HBM (128-byte row segments) and, as fp16 planes, into the LDS image of the second layer's A operand
    float* hb = a.H1 + (r0 + 4 * lh) * H1 + w * 32 * NT + li;
    char* awr = Aimg + 4 * lh * AROW + (w * 32 * NT + li) * 2;      // element (row rho + 4 lh, k = 64 w + 32 j + li): + rho * AROW + 64 j
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const lf_v4 sv = *reinterpret_cast<const lf_v4*>(totA + 8 * gq + 4 * lh);
      const lf_v4 ssv = *reinterpret_cast<const lf_v4*>(totA + 32 + 8 * gq + 4 * lh);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * gq + e;
        const int rho = 8 * gq + e;              // row inside the tile, minus the 4 * lh
        const float mean = ROW1 ? sv[e] : sv[e] * invH;
        const float rs = ROW1 ? ssv[e] : rsqrtf(fmaxf(0.f, ssv[e] * invH - mean * mean) + 1e-6f);
        const bool inb = r0 + rho + 4 * lh < a.M;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float xh = (z[j][r] - mean) * rs;
          const float h = act_fwd_t<ACT>(xh * gam[j] + bet[j]);
          // (nontemporal: h1 -- 67 MB per launch -- is next read by the weight-gradient launch three kernels later; written through
          //  the L2 it pushes out what the other chain's kernels are using.  Same-box A/B of two builds: 69.64 -> 68.75 ms per
          //  iteration.  The same hint on h2 (read by the next kernel: +0.65 ms), on the tail's H2 loads (+0.5) and dZ3 stores (+0.9)
          //  and on the weight-gradient producers' loads (+2.8: its column tiles share operand rows through the L2) is a loss.)
          // NTS (launches of at least 16384 rows: h1 is 32 MB and more, the size of the L2s): nontemporal stores.  h1 is next read by
          // the weight-gradient launch three kernels later; written through the L2 it pushes out what the other chain's kernels are
          // using.  Same-box A/B of two builds: 69.64 -> 68.75 ms per iteration at 32768 rows -- and 121.9 -> 124.4 at 4096 rows, where
          // h1 (8 MB per network) does stay in the L2 until it is read: plain stores there.  The same hint on h2 (read by the next
          // kernel: +0.65 ms), on the tail's H2 loads (+0.5) and dZ3 stores (+0.9) and on the weight-gradient producers' loads
          // (+2.8: its column tiles share operand rows through the L2) is a loss.
          if (inb && a.H1) {
            if (NTS) __builtin_nontemporal_store(h, &hb[(int64_t)rho * H1 + 32 * j]);
            else hb[(int64_t)rho * H1 + 32 * j] = h;
          }
          uint32_t p0, p1;
          bx_split2((inb ? h : 0.f) * X_ASCALE, 0.f, p0, p1);
          char* d = awr + rho * AROW + j * 64;
          *reinterpret_cast<uint16_t*>(d) = (uint16_t)p0;
          *reinterpret_cast<uint16_t*>(d + APLANE) = (uint16_t)p1;
        }
        __builtin_amdgcn_sched_barrier(0);     // one row at a time: hipcc otherwise runs all 32 ELU polynomials side by side and spills
      }
    }
    __syncthreads();      // the h1 image is complete
    L12_STAMP()
    // ---- second layer: h2 tile = act(h1 @ W2 + b2); barrier-free K loop, weight fragments PFX 16-k blocks ahead
    f32x16 acc[NT2];
#pragma unroll
    for (int j = 0; j < NT2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    constexpr int NB16 = H1 / 16;
    const char* ard = Aimg + li * AROW + lh * 16;                   // A fragment of 16-k block kb: + 32 kb (+ APLANE for the low plane)
#pragma unroll
    for (int u = 0; u < PFX; ++u)
#pragma unroll
      for (int j = 0; j < NT2; ++j)
#pragma unroll
        for (int p = 0; p < X_NP; ++p) bx[u][j][p] = W2x[(int64_t)u * w2_step + (j * X_NP + p) * 64];
#define RLX_L12_STEP(P, Q)                                                                                        \
  _Pragma("unroll") for (int j = 0; j < NT2; ++j)                                                                 \
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av[P]),                           \
                                                      __builtin_bit_cast(f16x8, bx[u][j][Q]), acc[j], 0, 0, 0);
#define RLX_L12_BLOCK(QU, REFILL)                                                                                 \
  {                                                                                                               \
    u32x4 av[X_NP];                                                                                               \
    const char* ab = ard + (QU) * 32;                                                                             \
    _Pragma("unroll") for (int p = 0; p < X_NP; ++p) av[p] = *reinterpret_cast<const u32x4*>(ab + p * APLANE);    \
    RLX_L12_STEP(0, 1)                                                                                            \
    RLX_L12_STEP(1, 0)                                                                                            \
    RLX_L12_STEP(0, 0)                                                                                            \
    if (REFILL) {                                                                                                 \
      _Pragma("unroll") for (int j = 0; j < NT2; ++j) _Pragma("unroll") for (int p = 0; p < X_NP; ++p)            \
          bx[u][j][p] = W2x[(int64_t)((QU) + PFX) * w2_step + (j * X_NP + p) * 64];                               \
      if (PFZ) __builtin_amdgcn_sched_barrier(0);                                                                 \
    } else if (PFZ) {      /* wrap: column tile u of block 0 of the first-layer image, for the next tile's z1 */      \
      _Pragma("unroll") for (int p = 0; p < X_NP; ++p) bx[u][0][p] = w1n[(u * X_NP + p) * 64];                    \
      __builtin_amdgcn_sched_barrier(0);   /* the refill stays behind ITS products: no drained wait in front of the next block */ \
    }                                                                                                             \
  }
    // (the last PFX blocks are peeled: with the refill behind `if (q + u + PFX < NB16)` the loads outstanding at the loop header
    //  depend on the path and hipcc waits with vmcnt(0) every other block -- half the prefetch depth)
    gfrag_t w1n = nullptr;                           // PFZ: the first-layer image the peeled blocks wrap into
#pragma unroll 1
    for (int q = 0; q < NB16 - PFX; q += PFX) {      // (not unrolled: hipcc otherwise hoists all 32 blocks' operand loads and spills)
#pragma unroll
      for (int u = 0; u < PFX; ++u) RLX_L12_BLOCK(q + u, true)
    }
    if constexpr (PFZ) w1n = w1_image();
#pragma unroll
    for (int u = 0; u < PFX; ++u) RLX_L12_BLOCK(NB16 - PFX + u, false)
#undef RLX_L12_BLOCK
#undef RLX_L12_STEP
    if constexpr (PFZ) {
      // block 1 of the first-layer image for the next tile's z1 (a tile without a successor fetches it for nothing: no branch, the
      // waits stay counted), then the next tile's observations -- requested a whole K loop ago -- into the other buffer
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int p = 0; p < X_NP; ++p) w1r[j][p] = w1n[w1_step + (j * X_NP + p) * 64];
      if (has_next) x_store(buf ^ 1);       // (its last readers finished before this tile's first barrier; the loop-top barrier publishes it)
    }
    L12_STAMP()
    {
      const float so = X_AINV * X_WINV;
      float* cb = a.H2 + (r0 + 4 * lh) * N2 + w * 32 * NT2 + li;
#pragma unroll
      for (int j = 0; j < NT2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rho = (r & 3) + 8 * (r >> 2);
          if (r0 + rho + 4 * lh < a.M) cb[(int64_t)rho * N2 + 32 * j] = act_fwd_t<ACT>(fmaf(acc[j][r], so, b2v[j]));
        }
    }
    L12_STAMP()
    L12_WALL(15)
  }
#undef L12_STAMP
#undef L12_WALL
