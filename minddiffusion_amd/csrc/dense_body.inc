// The tile program of the lean dense kernel (dense.hip), included twice: MDX_DENSE_SEG 0 = dense_kernel, the one-source kernel under
// the name and with the code it has always had; 1 = dense_seg_kernel, the K-segmented A operand (SEG, see dense.hip).  One source, two
// __global__ entry points.  Why not a sixth template parameter on dense_kernel: the one-source kernels keep their symbols (five template
// arguments; tests/test_host_cpu.py finds them by name to count their prefetch loads against their first wait).  Why not a shared
// __device__ body behind two wrappers: tried, and it moved the register allocation of a third of the one-source instantiations.
#if MDX_DENSE_SEG
template <int BM, int BN, int NS, int PF>
__global__ __launch_bounds__(256, 2) void dense_seg_kernel(const GemmParams p) {
    constexpr bool XA = false, SEG = true;
#else
template <int BM, int BN, int NS, int PF, bool XA = false>
__global__ __launch_bounds__(256, 2) void dense_kernel(const GemmParams p) {
    constexpr bool SEG = false;
#endif
    mdx_kernarg_touch<sizeof(GemmParams)>();
    constexpr int NW = 4;
    // Wave layout, chosen by the tile: BN a multiple of 64 -> four waves 2 x 2, a wave's tile is BM / 2 x BN / 2; otherwise (BN = 160: 80
    // columns are no whole number of 32 x 32 MFMA tiles) four waves 4 x 1, a wave's tile is BM / 4 = 32 rows x BN columns: one A fragment
    // and BN / 32 = 5 B fragments for five MFMAs per 16-deep k-step (1.2 KB of LDS reads per MFMA; the 128 x 64 tile reads 1.5 KB).
    constexpr bool W41 = BN % 64 != 0;
    static_assert(!W41 || (BM == 128 && BN % 32 == 0 && !XA && PF <= 1), "4 x 1 wave layout: 128-row tiles, prefetch level 0 / 1");
    static_assert(!SEG || (!W41 && !XA && PF <= 1), "K-segmented A: the 2 x 2 wave layouts, no cross-attention epilogue, prefetch level 0 / 1");
    constexpr int WROWS = W41 ? BM / 4 : BM / 2;      // rows per wave row
    constexpr int TM = WROWS / 32;
    constexpr int TN = W41 ? BN / 32 : BN / 64;
    constexpr int ROWB = 128;                // bytes per LDS row
    constexpr int KS = 4;                    // MFMA k-steps per K tile
    constexpr int A_BYTES = BM * ROWB;
    constexpr int B_BYTES = BN * ROWB;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int AJ = BM / 8 / NW;          // A-tile DMA instructions per wave (8 rows each)
    constexpr int BJ = BN / 8 / NW;
    constexpr int LPT = AJ + BJ;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = W41 ? wave : wave >> 1, wn = W41 ? 0 : wave & 1;
    const int hi = lane >> 5;
    const int l31 = lane & 31;

    // ---- tile decode without a division.  SPREAD order (one row of M tiles): grid (tiles, splits) -- x runs fastest, so consecutive
    // workgroups (consecutive XCDs) take consecutive tiles exactly as gemm_kernel's 1-D grid does with its % and /.  Otherwise the
    // XCD-contiguous order: every XCD a contiguous run of tile ids.
    const int ntiles = p.tiles_m * p.tiles_n;
    const int tile_id = p.spread ? (int)blockIdx.x : (int)((blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3));
    if (tile_id >= ntiles) return;
    trace_mark(p, 0);
    int tile_m, tile_n;      // (inv_* = ceil(2^32 / d), 0 for d == 1: the quotient is then the id itself)
    if (p.n_fastest) {
        tile_m = p.inv_tiles_n ? (int)__umulhi((unsigned)tile_id, p.inv_tiles_n) : tile_id;
        tile_n = tile_id - tile_m * p.tiles_n;
    } else {
        tile_n = p.inv_tiles_m ? (int)__umulhi((unsigned)tile_id, p.inv_tiles_m) : tile_id;
        tile_m = tile_id - tile_n * p.tiles_m;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int split = (int)blockIdx.y;
    const int kt_begin = split * p.ktiles_per_split;
    const int kt_end = min(p.ktiles, kt_begin + p.ktiles_per_split);
    const int nt = kt_end - kt_begin;

    const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(p.a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(p.w, p.w_bytes);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rs_a2 = make_rsrc(SEG ? p.a2 : p.a, SEG ? p.a2_bytes : p.a_bytes);
    [[maybe_unused]] const int kt1 = p.c1 >> 6;      // SEG: first K tile of the second source

    // ---- loader offsets: fixed per lane for the whole launch, the K offset rides in the DMA's scalar operand (gemm_kernel's dense issue)
    const int lrow = lane >> 3, lchk = lane & 7;
    const unsigned row_bytes = (unsigned)p.c1 * 2u;
    unsigned a_voff[AJ], b_off[BJ];
    [[maybe_unused]] unsigned a_voff2[SEG ? AJ : 1];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int row = (wave * AJ + j) * 8 + lrow;
        const int m = m0 + row;
        a_voff[j] = m < p.M ? (unsigned)m * row_bytes + (unsigned)((lchk ^ ((row >> 1) & 7)) * 16) : MDX_OOB;
        if constexpr (SEG)
            a_voff2[j] = m < p.M ? (unsigned)m * ((unsigned)p.c2 * 2u) + (unsigned)((lchk ^ ((row >> 1) & 7)) * 16) : MDX_OOB;
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
        const int row = (wave * BJ + j) * 8 + lrow;
        if constexpr (W41) {
            // n0 = 160 tile_n is no panel boundary: the packed row is that of the GLOBAL weight row n0 + row.  n0 % 32 == 0, so the 8 rows of
            // one DMA stay inside a panel and (tile row >> 1) & 7 == (panel row >> 1) & 7: the pre-swizzled chunks land where the fragment
            // reads (swz from the tile-local row) expect them.  Rows past the padded N lie past w_bytes: the descriptor answers zero.
            const int grow = n0 + row;
            b_off[j] = (unsigned)(grow >> 6) * (unsigned)p.kt64 * 8192u + (unsigned)(((grow & 63) * 8 + lchk) * 16);
        } else {
            const int panel = (n0 >> 6) + (row >> 6);
            b_off[j] = (unsigned)panel * (unsigned)p.kt64 * 8192u + (unsigned)(((row & 63) * 8 + lchk) * 16);
        }
    }
    auto stage_tile = [&](int kt, int buf) {
        char* sbase = smem + buf * STAGE;
        if (SEG && kt >= kt1) {      // (block-uniform) the tile lies in the second source
            if constexpr (SEG) {
#pragma unroll
                for (int j = 0; j < AJ; ++j) dma16s(rs_a2, sbase + (wave * AJ + j) * 1024, a_voff2[j], (unsigned)(kt - kt1) * 128u);
            }
        } else {
#pragma unroll
            for (int j = 0; j < AJ; ++j) dma16s(rs_a, sbase + (wave * AJ + j) * 1024, a_voff[j], (unsigned)kt * 128u);
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) dma16s(rs_w, sbase + A_BYTES + (wave * BJ + j) * 1024, b_off[j], (unsigned)kt * 8192u);
    };
#pragma unroll
    for (int i = 0; i < NS - 1; ++i)
        if (i < nt) stage_tile(kt_begin + i, i);
    __builtin_amdgcn_sched_barrier(0);       // (nothing below may be scheduled in front of the first tiles' issue)
    trace_mark(p, 1);

    // ---- everything the epilogue reads from global memory, requested now: younger than the prologue DMAs, older than every refill.
    // All of it goes through buffer descriptors whose bounds check answers zero for what does not exist (no bias, no residual, no
    // LayerNorm fold, columns / rows past the edge): UNCONDITIONAL loads into registers nothing touches until the K loop is over --
    // a conditional load merged with a default value makes the compiler wait for it on the spot (seen in the ISA of the first form
    // of this kernel: s_waitcnt vmcnt(0) right behind the bias load, a full miss in front of the loop) -- and the SAME number of
    // loads in every wave, so that the first wait of the loop can count them (E below).
    constexpr int CPR = BN / 8, RPP = 256 / CPR, PASSES = BM / RPP;
    constexpr int NX = (PF >= 2 && !W41) ? (PASSES < 4 ? PASSES : 4) : 0;
    constexpr int LNR = PF >= 3 ? LNR_MAX : 0;
    constexpr int NT = PF == 1 || PF == 2 ? 2 : 0;       // touches (LayerNorm statistics lines, S[n] lines)
    constexpr int NB = BN == 128 ? 4 : 2;      // bias loads: 8 columns, + the 8 GEGLU gate columns on 128-column tiles; 4 x 1 layout: two
                                               // dwords, bias and S[n] of column n0 + tid (epilogue_w41 shares them through LDS)
    constexpr int E = NB + NX + LNR + (PF >= 2 ? 1 : 0) + NT;       // bias + residual rows + LayerNorm partials + S[n] + touches: EXACTLY the loads issued below (every
                                               // one is kept alive behind the loop; the first wait of the loop counts them)
    const bool geglu = p.epilogue == MDX_EPI_GEGLU;
    const __amdgpu_buffer_rsrc_t rs_bias = make_rsrc(p.bias, p.bias ? (unsigned)p.N * 4u : 0u);
    const __amdgpu_buffer_rsrc_t rs_res = make_rsrc(p.residual, (p.residual && !geglu) ? p.res_bytes : 0u);
    const bool ln_regs = PF >= 3 && p.ln_stats != nullptr && p.ln_nt <= LNR;
    const bool lns_regs = PF >= 2 && p.ln_stats != nullptr;
    const __amdgpu_buffer_rsrc_t rs_ln = make_rsrc(p.ln_stats, p.ln_stats ? (unsigned)p.M * (unsigned)p.ln_nt * 8u : 0u);
    const __amdgpu_buffer_rsrc_t rs_lns = make_rsrc(p.ln_s, p.ln_stats ? (unsigned)p.N * 4u : 0u);
    u32x4 braw[4] = {};
    if constexpr (W41) {
        const unsigned off = (tid < BN && n0 + tid < p.N) ? (unsigned)(n0 + tid) * 4u : MDX_OOB;
        braw[0][0] = __builtin_amdgcn_raw_buffer_load_b32(rs_bias, off, 0, 0);
        braw[1][0] = __builtin_amdgcn_raw_buffer_load_b32(rs_lns, off, 0, 0);      // (zero without a LayerNorm fold)
    } else {
        const int n = n0 + (geglu ? (tid & 7) : (tid % CPR)) * 8;
        const unsigned off = n < p.N ? (unsigned)n * 4u : MDX_OOB;
        braw[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_bias, off, 0, 0);
        braw[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_bias, off, 16, 0);
        if constexpr (NB == 4) {
            const unsigned goff = geglu ? off : MDX_OOB;       // GEGLU: the gate columns sit 64 further (gemm_bias_prefetch)
            braw[2] = __builtin_amdgcn_raw_buffer_load_b128(rs_bias, goff, 256, 0);
            braw[3] = __builtin_amdgcn_raw_buffer_load_b128(rs_bias, goff, 272, 0);
        }
    }
    u32x4 xraw[NX > 0 ? NX : 1];
    if constexpr (NX > 0) {
        const int n = n0 + (tid % CPR) * 8;
#pragma unroll
        for (int q = 0; q < NX; ++q) {
            const int m = m0 + tid / CPR + q * RPP;
            const unsigned off = (m < p.M && n < p.N) ? ((unsigned)m * (unsigned)p.residual_ld + (unsigned)n) * 2u : MDX_OOB;
            xraw[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, off, 0, 0);
        }
    }
    u32x2 lnraw[LNR > 0 ? LNR : 1];
    if constexpr (LNR > 0) {
        const unsigned base = (tid < BM && m0 + tid < p.M) ? (unsigned)(m0 + tid) * (unsigned)p.ln_nt * 8u : MDX_OOB;
#pragma unroll
        for (int j = 0; j < LNR; ++j)
            lnraw[j] = __builtin_amdgcn_raw_buffer_load_b64(rs_ln, (base != MDX_OOB && j < p.ln_nt) ? base : MDX_OOB, j * 8, 0);
    }
    unsigned lns_raw = 0u;
    if constexpr (PF >= 2)
        lns_raw = __builtin_amdgcn_raw_buffer_load_b32(rs_lns, (tid < BN && n0 + tid < p.N) ? (unsigned)(n0 + tid) * 4u : MDX_OOB, 0, 0);
    unsigned touch[2] = {0u, 0u};
    if constexpr (NT > 0) {      // rows whose partials stay in memory: one dword of every 128-byte line, the epilogue's fold then hits L2
        const int rows = min(BM, p.M - m0);
        const unsigned bytes = (unsigned)rows * (unsigned)p.ln_nt * 8u;
        const unsigned base = (unsigned)m0 * (unsigned)p.ln_nt * 8u;
        touch[0] = __builtin_amdgcn_raw_buffer_load_b32(rs_ln, (unsigned)tid * 128u < bytes ? base + (unsigned)tid * 128u : MDX_OOB, 0, 0);
        touch[1] = __builtin_amdgcn_raw_buffer_load_b32(rs_lns, (PF < 2 && tid < BN / 32 && n0 + tid * 32 < p.N) ? (unsigned)(n0 + tid * 32) * 4u : MDX_OOB, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int swz = (l31 >> 1) & 7;
    const int a_row_off = (wm * WROWS + l31) * ROWB;
    const int b_row_off = A_BYTES + (wn * (BN / 2) + l31) * ROWB;

    // ---- main loop: gemm_kernel's (NS-stage ring, counted vmcnt + raw barrier, refill issue first, fragment reads pinned, MFMAs)
    int rd = 0, wr = NS - 1;
    for (int t = 0; t < nt; ++t) {
        const int ahead = min(NS - 2, nt - 1 - t);
        if (t == 0) {      // the E epilogue prefetches are younger than every prologue tile: tile 0 has landed when at most they and the
                           // other prologue tiles are outstanding; from t = 1 on they count as landed (they had a K tile's time)
            if (NS >= 6 && ahead >= 4)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LPT + E) : "memory");
            else if (NS >= 5 && ahead == 3)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPT + E) : "memory");
            else if (NS >= 4 && ahead == 2)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT + E) : "memory");
            else if (NS >= 3 && ahead == 1)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT + E) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(E) : "memory");
        } else if (NS >= 6 && ahead >= 4)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LPT) : "memory");
        else if (NS >= 5 && ahead == 3)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPT) : "memory");
        else if (NS >= 4 && ahead == 2)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
        else if (NS >= 3 && ahead == 1)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (t == 0) trace_mark(p, 2);
        const char* sb = smem + rd * STAGE;
        constexpr bool ALLK = TM * TN <= 2;
        constexpr int FD = ALLK ? KS : 2;
        f16x8 af[FD][TM], bf[FD][TN];
        auto rdfrag = [&](auto slot_c, const int ks) {
            constexpr int slot = decltype(slot_c)::value;
            const int coff = (((2 * ks + hi) ^ swz) << 4);
#pragma unroll
            for (int i = 0; i < TM; ++i) af[slot][i] = *reinterpret_cast<const f16x8*>(sb + a_row_off + i * 32 * ROWB + coff);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[slot][j] = *reinterpret_cast<const f16x8*>(sb + b_row_off + j * 32 * ROWB + coff);
        };
        auto mfmas = [&](auto slot_c) {
            constexpr int slot = decltype(slot_c)::value;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[slot][j], af[slot][i], acc[i][j], 0, 0, 0);
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        if (t + NS - 1 < nt) stage_tile(kt_begin + t + NS - 1, wr);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ALLK) {
            using I2 = std::integral_constant<int, 2>;
            using I3 = std::integral_constant<int, 3>;
            rdfrag(I0{}, 0); rdfrag(I1{}, 1); rdfrag(I2{}, 2); rdfrag(I3{}, 3);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(I0{}); mfmas(I1{}); mfmas(I2{}); mfmas(I3{});
        } else {
            rdfrag(I0{}, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KS; ks += 2) {
                rdfrag(I1{}, ks + 1);
                __builtin_amdgcn_sched_barrier(0);
                mfmas(I0{});
                __builtin_amdgcn_sched_barrier(0);
                if (ks + 2 < KS) {
                    rdfrag(I0{}, ks + 2);
                    __builtin_amdgcn_sched_barrier(0);
                }
                mfmas(I1{});
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        rd = (rd + 1 == NS) ? 0 : rd + 1;
        wr = (wr + 1 == NS) ? 0 : wr + 1;
    }

    __syncthreads();      // all waves done with the ring before the epilogue reuses it
    trace_mark(p, 3);
    // unpack the prefetches (the loop's last wait was vmcnt(0): everything has landed).  Every prefetched register is named here
    // once, unconditionally: none of the E loads can be removed as dead, whatever the epilogue instantiation reads
#pragma unroll
    for (int q = 0; q < NB; ++q) asm volatile("" ::"v"(braw[q]));
#pragma unroll
    for (int q = 0; q < NX; ++q) asm volatile("" ::"v"(xraw[q]));
#pragma unroll
    for (int j = 0; j < LNR; ++j) asm volatile("" ::"v"(lnraw[j]));
    if constexpr (PF >= 2) asm volatile("" ::"v"(lns_raw));
#pragma unroll
    for (int q = 0; q < NT; ++q) asm volatile("" ::"v"(touch[q]));
    float bpre[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 f = __builtin_bit_cast(f32x4, braw[q]);
        bpre[4 * q] = f[0]; bpre[4 * q + 1] = f[1]; bpre[4 * q + 2] = f[2]; bpre[4 * q + 3] = f[3];
    }
    Row8Extras xpre[NX > 0 ? NX : 1];
#pragma unroll
    for (int q = 0; q < NX; ++q) xpre[q].res = __builtin_bit_cast(f16x8, xraw[q]);
    // LayerNorm fold: this thread's row statistics from the partials it holds, added in partial order (the order gemm_ln_row_fold
    // uses; the zeros of the slots past ln_nt change nothing: same bits)
    float ln_pre[2];
    {
        float su = 0.f, sq = 0.f;
#pragma unroll
        for (int j = 0; j < LNR; ++j) {
            const float2 v = __builtin_bit_cast(float2, lnraw[j]);
            su += v.x;
            sq += v.y;
        }
        const float inv = 1.0f / (float)p.K;
        const float mean = su * inv;
        float var = sq * inv - mean * mean;
        var = var < 0.f ? 0.f : var;
        ln_pre[0] = mean;
        ln_pre[1] = rsqrtf(var + p.ln_eps);
    }
    const float lns_pre = __builtin_bit_cast(float, lns_raw);
    // (xpre is read only where the descriptor has a residual; the GEGLU store path fetches nothing)
    if constexpr (XA) {
        static_assert(BN == 64, "cross-attention epilogue: one 64-wide head per tile");
        // the head's K / V^T tiles -> LDS behind the staging area, in flight while the accumulators are corrected and staged
        constexpr int XOFF = ((BM * 72 * 2 + 2 * BM * 4 + BN * 4 + 1023) / 1024) * 1024;
        char* xs = smem + XOFF;
        // (two slots; a context of more than two tiles re-stages them pair by pair inside xattn_tile_epilogue.  Offsets stay in 32 bits:
        // xa_len <= 1024 keys of N <= 2^20 halves, checked by the resolver's 2 GiB bound)
        const int bsamp = m0 / p.HoWo, head = n0 >> 6;
        const f16* kb = p.xa_k + (size_t)bsamp * p.xa_cap * p.N + head * 64;
        const f16* vb = p.xa_vt + ((size_t)bsamp * p.N + head * 64) * p.xa_cap;
        const __amdgpu_buffer_rsrc_t rs_k = make_rsrc(kb, (unsigned)(((size_t)(p.xa_len - 1) * p.N + 64) * 2));
        const __amdgpu_buffer_rsrc_t rs_v = make_rsrc(vb, (unsigned)((size_t)64 * p.xa_cap * 2));
        const int ntile = (p.xa_len + 63) >> 6;
        auto stage_pair = [&](const int t0) {
            const int t1 = t0 + 2 < ntile ? t0 + 2 : ntile;
            for (int t = t0; t < t1; ++t) {
                char* slot = xs + (t & 1) * 16384;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int inst = wave * 2 + j;
                    const int krow = inst * 8 + (lane >> 3);
                    const int kchunk = (lane & 7) ^ ((krow >> 1) & 7);
                    const int key = t * 64 + krow;
                    dma16(rs_k, slot + inst * 1024, key < p.xa_len ? (unsigned)(((size_t)key * p.N + kchunk * 8) * 2) : MDX_OOB);
                    const int vrow = inst * 8 + (lane >> 3);
                    const unsigned vchunk = (unsigned)((lane & 7) ^ ((vrow >> 1) & 7));
                    const int kc = t * 64 + (int)vchunk * 8;
                    dma16(rs_v, slot + 8192 + inst * 1024, kc < p.xa_cap ? (unsigned)(((size_t)vrow * p.xa_cap + kc) * 2) : MDX_OOB);
                }
            }
        };
        stage_pair(0);
        gemm_epilogue<BM, BN, true, NW, LinearRows, NX, 3>(p, acc, smem, LinearRows{m0}, n0, split, bpre, tile_m, tile_id, ln_pre, &lns_pre, xpre,
                                                           ln_regs, lns_regs);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();      // K / V^T of every wave's DMAs landed (the staged q tile was ordered by the epilogue's own barrier)
        xattn_tile_epilogue<BM>(p, smem, xs, m0, n0, stage_pair);
    } else if constexpr (W41) {
        epilogue_w41<BM, BN>(p, acc[0], smem, m0, n0, bpre[0], bpre[4]);
    } else {
        gemm_epilogue<BM, BN, true, NW, LinearRows, NX, LEAN_EPI ? 1 : 0>(p, acc, smem, LinearRows{m0}, n0, split, bpre, tile_m, tile_id, ln_pre,
                                                                  &lns_pre, xpre, ln_regs, lns_regs);
    }
    trace_mark(p, 4);
}
