// The LDS-tiled MFMA GEMM (gemm_f32_mfma_kernel, the path of the largest shapes) and its split-K reduce.  Included by
// tnn_gemm.hip inside its anonymous namespace, after tnn_gemm_args.h; launch_cfg / gemm_f32 in tnn_gemm.hip choose the tile.
#pragma once

// K1: GEMM for the three contractions of ops.dot_ (core/ops.py:151 NN, :157 NT, :160 TN) with the
// fused epilogues of K8.  fp32 path = v_mfma_f32_32x32x2_f32 (exact f32, 256 FLOP/clk/CU, 157 TF
// chip peak), LDS double-buffered, one barrier per K-tile, register-staged prefetch of the next
// tile, XCD-aware tile order.  No operand is ever transposed in memory: each operand is staged in
// the layout it already has and only the LDS read pattern differs.
//
// Operand layouts ("KC" = K is the contiguous axis of the stored matrix):
//     NN: A[M,K] KC      B[K,N] N-contiguous
//     NT: A[M,K] KC      B[N,K] KC
//     TN: A[K,M] M-contig B[K,N] N-contiguous
// LDS images:  KC operand      -> [rows][BK+4]   fragment = one ds_read_b128 per 8-deep k-chunk
//                                  (row stride 144 B: conflict-free for the 16-lane b128 groups)
//              MN-contig operand -> [BK][rows]    fragment = 4 ds_read_b32 (32 consecutive dwords)
// k-assignment inside an 8-deep chunk: lanes 0-31 hold k = 0..3, lanes 32-63 hold k = 4..7; MFMA j
// contracts {j, 4+j}.  A and B use the same assignment, so the sum is complete; only the fp32
// summation order differs from a sequential loop (tolerance, not bit-exactness, is the f32 bar).

// VEC = both operands allow 16-B loads (aligned base, leading dimension and contiguous extent multiples
// of 4): the main loop is then branch-free — per-thread source pointers, row-validity flags and LDS
// offsets are computed once before the loop, out-of-range rows read a clamped (valid) address and are
// zeroed with a select, and only the last, partial K-tile goes through the guarded element-wise loader.
// VEC = false is the fully guarded element-wise variant for odd shapes / unaligned views.
template <int BM, int BN, int BK, int WM, int WN, bool AKC, bool BKC, bool VEC>
__global__ __launch_bounds__(WM* WN * 64) void gemm_f32_mfma_kernel(GemmArgs g) {
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NI = TN / 32;
    constexpr int SA = AKC ? BK + 4 : BM;          // LDS row stride (floats)
    constexpr int SB = BKC ? BK + 4 : BN;
    constexpr int A_ELEMS = AKC ? BM * SA : BK * SA;
    constexpr int B_ELEMS = BKC ? BN * SB : BK * SB;
    constexpr int A_F4 = BM * BK / 4 / NT;         // float4 per thread per tile
    constexpr int B_F4 = BN * BK / 4 / NT;
    static_assert(A_F4 >= 1 && B_F4 >= 1, "tile too small for the block");
    static_assert(BK % 8 == 0, "BK must be a multiple of 8");

    __shared__ __attribute__((aligned(16))) float lds[2 * (A_ELEMS + B_ELEMS)];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int l31 = lane & 31, lhi = lane >> 5;
    // Debug build only (make trace -> libtnn_hip_trace.so, tools/gemm_block_timeline.py): thread 0 of every
    // workgroup leaves four 100 MHz timestamps (entry, K loop start, K loop end, stores acknowledged) and its
    // HW_ID / XCC_ID in a host-supplied buffer, 8 words per workgroup.  The entry record — HW_ID and the first stamp, one
    // guarded block in the compiled kernel — is no plain clock stamp and keeps its #ifdef; the other three go through the hook.
#define TNN_TRACE(i) TNN_GEMM_STAMP(g.trace, (size_t)blockIdx.x, 8, g.trace ? ~(size_t)0 : 0, i)     // every row, if there is a buffer
#ifdef TNN_GEMM_TRACE
    if (tid == 0 && g.trace) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g.trace[(size_t)blockIdx.x * 8 + 4] = ((unsigned long long)xcc << 32) | hw;
        g.trace[(size_t)blockIdx.x * 8] = wall_clock64();
    }
#endif
    // tile order: each XCD (private 4 MB L2) gets a contiguous range of ids (xcd_remap); inside the range the
    // ids sweep N for a GROUP of 8 M-tiles at a time, so the group's A panels stay L2-resident while the B
    // panels stream through once (measured before this: 469 MB fetched by the 4096x4096x512 TN GEMM for
    // 16 MB of inputs, every A panel was evicted between its reuses)
    const int nb = g.tiles_m * g.tiles_n;
    const int t = xcd_remap((int)blockIdx.x, nb);
    const int GROUP_M = g.group_m;                     // 8 (TNN_GEMM_GROUP_M: the raster sweep of tools/gemm_sweep.py)
    const int per_group = GROUP_M * g.tiles_n;
    const int first_m = (t / per_group) * GROUP_M;
    const int gsz = min(g.tiles_m - first_m, GROUP_M);
    const int64_t m0 = (int64_t)(first_m + (t % per_group) % gsz) * BM;
    const int64_t n0 = (int64_t)((t % per_group) / gsz) * BN;
    const int64_t kbeg = (int64_t)blockIdx.z * g.k_per_split;
    const int64_t kend = min(g.K, kbeg + g.k_per_split);
    const int nk = (int)((kend - kbeg + BK - 1) / BK);
    const int nk_full = (int)((kend - kbeg) / BK);      // tiles that need no K guard

    // ---- per-thread staging geometry, fixed for the whole K loop
    // element (row, c4) of the tile: KC operand -> row = m/n index, c4 = k/4;  MN-contig -> row = k, c4 = m/4
    // fast loader addressing = wave-uniform base (advances by a scalar add per K-tile) + a per-thread 32-bit byte
    // offset that never changes (the host takes this kernel's VEC variant only for operands below 4 GiB)
    uint32_t a_off[A_F4], b_off[B_F4];
    int a_dst[A_F4], b_dst[B_F4];
    int a_row[A_F4], a_c4[A_F4], b_row[B_F4], b_c4[B_F4];
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
        const int f = tid + i * NT;
        a_row[i] = AKC ? f / (BK / 4) : f / (BM / 4);
        a_c4[i] = AKC ? f % (BK / 4) : f % (BM / 4);
        a_dst[i] = a_row[i] * SA + a_c4[i] * 4;
        if constexpr (AKC) {
            const int64_t gm = m0 + a_row[i];
            a_off[i] = (uint32_t)(((gm < g.M ? gm : 0) * g.lda + a_c4[i] * 4) * 4);
        } else {
            const int64_t gm = m0 + a_c4[i] * 4;       // VEC: M % 4 == 0, a float4 is wholly in or out of range
            a_off[i] = (uint32_t)((a_row[i] * g.lda + (gm < g.M ? gm : 0)) * 4);
        }
    }
#pragma unroll
    for (int i = 0; i < B_F4; ++i) {
        const int f = tid + i * NT;
        b_row[i] = BKC ? f / (BK / 4) : f / (BN / 4);
        b_c4[i] = BKC ? f % (BK / 4) : f % (BN / 4);
        b_dst[i] = b_row[i] * SB + b_c4[i] * 4;
        if constexpr (BKC) {
            const int64_t gn = n0 + b_row[i];
            b_off[i] = (uint32_t)(((gn < g.N ? gn : 0) * g.ldb + b_c4[i] * 4) * 4);
        } else {
            const int64_t gn = n0 + b_c4[i] * 4;
            b_off[i] = (uint32_t)((b_row[i] * g.ldb + (gn < g.N ? gn : 0)) * 4);
        }
    }
    const int64_t a_step = (AKC ? (int64_t)BK : (int64_t)BK * g.lda) * 4;   // bytes per K-tile
    const int64_t b_step = (BKC ? (int64_t)BK : (int64_t)BK * g.ldb) * 4;
    const char* const a_base = reinterpret_cast<const char*>(g.A) + (AKC ? kbeg : kbeg * g.lda) * 4;
    const char* const b_base = reinterpret_cast<const char*>(g.B) + (BKC ? kbeg : kbeg * g.ldb) * 4;

    float4 ra[A_F4], rb[B_F4];

    // fast loader: full K-tile, 16-B loads, no branches and NO use of the loaded value (a select here would
    // put an s_waitcnt right behind the loads and expose the whole global latency before the MFMAs).  Rows /
    // columns beyond M / N read a clamped, valid address: what they load only ever reaches accumulator rows /
    // columns >= M / N, which the epilogue never stores (an output row depends on its own A row only).
    // buffer loads: resource (4 SGPRs) + constant per-thread VGPR offset + a scalar offset that advances per K-tile —
    // no vector address arithmetic at all in the loop, and a single address VGPR per load
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(a_base), 0, 0xffffffffu, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(b_base), 0, 0xffffffffu, 0x00020000);
    auto load_full = [&](int kt) {
        const uint32_t at = (uint32_t)kt * (uint32_t)a_step, bt = (uint32_t)kt * (uint32_t)b_step;   // wave-uniform
#pragma unroll
        for (int i = 0; i < A_F4; ++i)
            ra[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_off[i], at, 0));
#pragma unroll
        for (int i = 0; i < B_F4; ++i)
            rb[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_off[i], bt, 0));
    };
    // guarded loader: element-wise bounds on every axis (K tail, odd shapes, unaligned operands)
    auto load_guarded = [&](int kt) {
        const int64_t k0 = kbeg + (int64_t)kt * BK;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (AKC) {
                const int64_t gm = m0 + a_row[i], gk = k0 + a_c4[i] * 4;
                if (gm < g.M) {
                    const float* p = g.A + gm * g.lda + gk;
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (gk + j < kend) e[j] = p[j];
                }
            } else {
                const int64_t gk = k0 + a_row[i], gm = m0 + a_c4[i] * 4;
                if (gk < kend) {
                    const float* p = g.A + gk * g.lda + gm;
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (gm + j < g.M) e[j] = p[j];
                }
            }
            ra[i] = make_float4(e[0], e[1], e[2], e[3]);
        }
#pragma unroll
        for (int i = 0; i < B_F4; ++i) {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (BKC) {
                const int64_t gn = n0 + b_row[i], gk = k0 + b_c4[i] * 4;
                if (gn < g.N) {
                    const float* p = g.B + gn * g.ldb + gk;
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (gk + j < kend) e[j] = p[j];
                }
            } else {
                const int64_t gk = k0 + b_row[i], gn = n0 + b_c4[i] * 4;
                if (gk < kend) {
                    const float* p = g.B + gk * g.ldb + gn;
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (gn + j < g.N) e[j] = p[j];
                }
            }
            rb[i] = make_float4(e[0], e[1], e[2], e[3]);
        }
    };
    auto load_tile = [&](int kt) {
        if (VEC && kt < nk_full) load_full(kt);
        else load_guarded(kt);
    };

    auto store_tile = [&](int buf) {
        float* As = lds + buf * (A_ELEMS + B_ELEMS);
        float* Bs = As + A_ELEMS;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) *reinterpret_cast<float4*>(As + a_dst[i]) = ra[i];
#pragma unroll
        for (int i = 0; i < B_F4; ++i) *reinterpret_cast<float4*>(Bs + b_dst[i]) = rb[i];
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // LDS fragment base offsets (floats), fixed for the whole loop
    const int a_frag = AKC ? (wm * TM + l31) * SA + lhi * 4 : (lhi * 4) * SA + wm * TM + l31;
    const int b_frag = BKC ? (wn * TN + l31) * SB + lhi * 4 : (lhi * 4) * SB + wn * TN + l31;
    constexpr int KK = BK / 8;

    // Fragment registers: one slot per 8-deep chunk of the K-tile, filled TWO chunks ahead of their MFMAs.
    float af[KK][MI][4], bf[KK][NI][4];
    auto read_frag = [&](int buf, int kk) {
        const float* As = lds + buf * (A_ELEMS + B_ELEMS);
        const float* Bs = As + A_ELEMS;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            if constexpr (AKC) {
                float4 v = *reinterpret_cast<const float4*>(As + a_frag + i * 32 * SA + kk * 8);
                af[kk][i][0] = v.x; af[kk][i][1] = v.y; af[kk][i][2] = v.z; af[kk][i][3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) af[kk][i][j] = As[a_frag + (kk * 8 + j) * SA + i * 32];
            }
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if constexpr (BKC) {
                float4 v = *reinterpret_cast<const float4*>(Bs + b_frag + i * 32 * SB + kk * 8);
                bf[kk][i][0] = v.x; bf[kk][i][1] = v.y; bf[kk][i][2] = v.z; bf[kk][i][3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[kk][i][j] = Bs[b_frag + (kk * 8 + j) * SB + i * 32];
            }
        }
    };
    auto mfma_chunk = [&](int kk) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    // operands SWAPPED: the block accumulates (A B)^T, i.e. lane l31 owns output ROW l31 of the block and
                    // its registers (r & 3) hold 4 CONSECUTIVE COLUMNS — the epilogue leaves through 16-B stores
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[kk][ni][j], af[kk][mi][j],
                                                                       acc[mi][ni], 0, 0, 0);
    };

    // Software pipeline — one barrier per K-tile and no exposed LDS or global latency in steady state.
    // Chunk c runs the MFMAs of fragment c and, BEFORE them, issues the LDS reads of the fragment used two
    // chunks later (sched_barrier(0) pins "memory ops first, then the chunk's MFMAs": left alone hipcc sinks
    // the reads below the MFMAs and then drains them in front of the barrier):
    //   chunk 0 : write tile kt+1 to the other buffer (its global loads were issued a whole tile ago),
    //             issue the global loads of tile kt+2, read F(kt,2) and F(kt,3)           | MFMA F(kt,0)
    //   chunk 1 :                                                                         | MFMA F(kt,1)
    //   ---- s_barrier ---- (pinned, see pinned_barrier)
    //   chunk 2 : read F(kt+1,0), F(kt+1,1) from the other buffer                         | MFMA F(kt,2)
    //   chunk 3 :                                                                         | MFMA F(kt,3)
    // (the tail loop keeps the older placement: F(kt,3) in chunk 1, F(kt+1,1) in chunk 3 — same register slots)
    // Hazards: the buffer written in chunk 0 of tile kt was last read in chunks 0-1 of tile kt-1, i.e. before
    // the barrier of tile kt-1 that every wave has passed; it is first read after the barrier of tile kt,
    // which every wave reaches after its own writes.
    static_assert(KK == 4, "the pipeline below is written for BK = 32");
    if (nk > 0) {
        load_tile(0);
        store_tile(0);
        if (nk > 1) load_tile(1);
    }
    __syncthreads();
    if (nk > 0) {
        read_frag(0, 0);
        read_frag(0, 1);
    }

    // Interleave pattern for one chunk: each MFMA (64 cycles on the pipe) is followed by a few of the chunk's
    // memory / address instructions, so that they issue in the MFMA's shadow instead of in a burst between MFMA
    // groups (masks: 0x8 MFMA, 0x2 VALU, 0x4 SALU, 0x20 VMEM read, 0x100 DS read, 0x200 DS write).
    constexpr int NMF = MI * NI * 4;           // MFMAs per chunk
#define TNN_INTERLEAVE_LIGHT()                                             \
    _Pragma("unroll") for (int q = 0; q < NMF; ++q) {                      \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                 \
    }
#define TNN_INTERLEAVE_HEAVY()                                             \
    _Pragma("unroll") for (int q = 0; q < NMF; ++q) {                      \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                 \
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                 \
    }

    // The barrier as the compiler must see it: hipcc hoists the register-only MFMAs of chunks 2-3 above a plain
    // __syncthreads() (nothing orders them against it), which leaves the post-barrier LDS reads with no MFMAs to hide
    // behind.  Empty asm statements that "redefine" the fragments of chunks 2-3 right after the barrier tie those
    // MFMAs to it (volatile asm statements keep their order).  lgkmcnt(0): this wave's tile stores have landed.
    auto pinned_barrier = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int kk = 2; kk < 4; ++kk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < MI; ++i) asm volatile("" : "+v"(af[kk][i][j]));
#pragma unroll
                for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(bf[kk][i][j]));
            }
        }
    };
    // steady state: tiles kt+1 and kt+2 exist and tile kt+2 is a full, vector-loadable tile -> no branches.
    // Two tiles per trip with the buffer index a compile-time constant: every LDS address is then a loop-invariant
    // register plus an immediate offset (no per-tile address arithmetic next to the MFMAs).
    TNN_TRACE(1);
    int kt = 0;
    const int n_steady = VEC ? (nk_full - 2 < nk - 2 ? nk_full - 2 : nk - 2) : 0;
#define TNN_STEADY_TILE(CUR, KT)                                           \
    store_tile((CUR) ^ 1);                                                 \
    load_full((KT) + 2);                                                   \
    read_frag((CUR), 2);                                                   \
    read_frag((CUR), 3);                                                   \
    mfma_chunk(0);                                                         \
    TNN_INTERLEAVE_HEAVY();                                                \
    __builtin_amdgcn_sched_barrier(0);                                     \
    mfma_chunk(1);                                                         \
    __builtin_amdgcn_sched_barrier(0);                                     \
    pinned_barrier();                                                      \
    __builtin_amdgcn_sched_barrier(0);                                     \
    read_frag((CUR) ^ 1, 0);                                               \
    read_frag((CUR) ^ 1, 1);                                               \
    mfma_chunk(2);                                                         \
    TNN_INTERLEAVE_LIGHT();                                                \
    __builtin_amdgcn_sched_barrier(0);                                     \
    mfma_chunk(3);                                                         \
    __builtin_amdgcn_sched_barrier(0);
    for (; kt + 1 < n_steady; kt += 2) {
        TNN_STEADY_TILE(0, kt)
        TNN_STEADY_TILE(1, kt + 1)
    }
#undef TNN_STEADY_TILE
#undef TNN_INTERLEAVE_LIGHT
#undef TNN_INTERLEAVE_HEAVY

    // remaining tiles (the last two, a partial K tail, or every tile of the guarded variant): same pipeline
    // with its conditionals
    for (; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool has1 = kt + 1 < nk, has2 = kt + 2 < nk;
        if (has1) store_tile(cur ^ 1);
        if (has2) load_tile(kt + 2);
        read_frag(cur, 2);
        __builtin_amdgcn_sched_barrier(0);
        mfma_chunk(0);
        __builtin_amdgcn_sched_barrier(0);

        read_frag(cur, 3);
        __builtin_amdgcn_sched_barrier(0);
        mfma_chunk(1);
        __builtin_amdgcn_sched_barrier(0);

        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);

        if (has1) read_frag(cur ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfma_chunk(2);
        __builtin_amdgcn_sched_barrier(0);

        if (has1) read_frag(cur ^ 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_chunk(3);
        __builtin_amdgcn_sched_barrier(0);
    }

    TNN_TRACE(2);
    // epilogue: with the swapped operands lane l31 holds ROW l31 of each 32x32 block and register r the column
    // (r & 3) + 8 (r >> 2) + 4 lhi: four consecutive columns per register quad -> one 16-B store per quad (4 store
    // instructions per block instead of 16 dword stores; 8 instead of 32 per wave for the 128x64 tile)
    if (g.epi == EPI_ADAM) {
        // The tile is a weight gradient: Adam (core/optimizer.py:67-79, the maths of adam_kernel in tnn_fused.hip) updates the
        // matching block of p / m / v here, 16 B per lane and array, and the gradient goes to C only if the caller wants it
        // stored.  The fp32 product is MFMA-bound, so the optimizer's 24 B per parameter ride on an otherwise idle memory
        // system (host side guarantees: splits == 1, 16-B aligned arrays, ldc % 4 == 0, N % 4 == 0).
        if (g.ad_guard != nullptr && *g.ad_guard != 0) return;
        const float ic1 = (float)(1.0 / (1.0 - g.ad_pows[0])), ic2 = (float)(1.0 / (1.0 - g.ad_pows[1]));
        const float omb1 = 1.f - g.ad_b1, omb2 = 1.f - g.ad_b2, lr = g.ad_lr, eps = g.ad_eps;
        if (!BKC && g.cs_db != nullptr && blockIdx.z == 0 && (int)(m0 / BM) == (int)(n0 / BN) % g.tiles_m) {
            // ONE workgroup per tile column (tile row = column index mod tiles_m: spread over the XCDs and over the launch's
            // duration — with all of them in tile row 0 they sat on two XCDs) also produces db = column sums of B (= dz,
            // MN-contiguous: the TN form) for its BN columns and applies
            // Adam to the bias block (core/ops.py:52-54 + core/optimizer.py:67-79).  The K x BN panel was streamed through
            // this workgroup a moment ago (L2 hits); summing it again HERE, outside the K loop, costs the 64 workgroups of the
            // row a few microseconds and leaves the MFMA loop alone (a first version added f64 adds on the B fragments
            // inside the loop's wave-uniform branch: the dW launch went from 162 to 182 us — the interleave pattern of the
            // loop does not survive extra VALU work).  f64 accumulation like every reduction of the library (tnn_reduce).
            constexpr int C4 = BN / 4, PARTS = NT / C4;            // 16-B loads: thread = (4 columns, one of PARTS row classes)
            // the partial sums meet in the operand buffers (free after the K loop): NO LDS of their own — 8 KB more per
            // workgroup took the kernel from 3 to 2 workgroups per CU, for every product of the library (measured: +3 %)
            static_assert(NT % C4 == 0 && PARTS * BN * 8 <= 2 * (A_ELEMS + B_ELEMS) * 4, "column-sum lanes / LDS");
            __syncthreads();                                    // every wave is done with the last tile's fragments
            double (*cs_part)[BN] = reinterpret_cast<double (*)[BN]>(lds);
            const int c4 = tid % C4, part4 = tid / C4;
            double a4[4] = {0.0, 0.0, 0.0, 0.0};
            if (n0 + 4 * c4 + 3 < g.N && g.vecB) {
                const float* bp = g.B + n0 + 4 * c4;
                constexpr int UN = 8;                               // independent loads in flight per thread
                for (int64_t k0 = part4; k0 < g.K; k0 += (int64_t)PARTS * UN) {
                    f32x4 v[UN];
#pragma unroll
                    for (int u = 0; u < UN; ++u) {
                        const int64_t k = k0 + (int64_t)u * PARTS;
                        v[u] = k < g.K ? *reinterpret_cast<const f32x4*>(bp + k * g.ldb) : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int u = 0; u < UN; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) a4[e] += (double)v[u][e];
                }
            } else {
                for (int e = 0; e < 4; ++e) {
                    const int64_t gc = n0 + 4 * c4 + e;
                    if (gc < g.N)
                        for (int64_t k = part4; k < g.K; k += PARTS) a4[e] += (double)g.B[k * g.ldb + gc];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) cs_part[part4][4 * c4 + e] = a4[e];
            __syncthreads();
            const int col = tid % BN, part = tid / BN;
            const int64_t gcol = n0 + col;
            if (part == 0 && gcol < g.N) {
                double t = 0.0;
#pragma unroll
                for (int q = 0; q < PARTS; ++q) t += cs_part[q][col];
                const float sum = (float)t;
                g.cs_db[gcol] = sum;
                if (g.cs_p != nullptr) {
                    float mi = g.cs_m[gcol], vi = g.cs_v[gcol];
                    mi = mi + omb1 * (sum - mi);
                    vi = vi + omb2 * (sum * sum - vi);
                    g.cs_m[gcol] = mi;
                    g.cs_v[gcol] = vi;
                    g.cs_p[gcol] = g.cs_p[gcol] + (-lr * (mi * ic1) / (sqrtf(vi * ic2) + eps));
                }
            }
            __syncthreads();
        }
        constexpr int TS = BN + 4;                                    // LDS row stride of the staged tile (floats)
        if constexpr (BM * TS <= 2 * (A_ELEMS + B_ELEMS) && (BN / 4) <= NT && NT % (BN / 4) == 0) {
            // Interior tiles leave through LDS.  In the accumulator layout a lane owns a ROW and 4 consecutive columns: a 16-B
            // access per lane touches 32 rows x 32 B per instruction — fine for the one store of a plain product, but the
            // optimizer adds three loads and three stores per element (measured: the step got SLOWER, 0.85 -> 1.00 ms, with
            // that pattern).  Staged row-major, a wave instruction covers 4 whole 256-B tile rows.
            if (m0 + BM <= g.M && n0 + BN <= g.N) {                   // block-uniform
                __syncthreads();                                      // every wave is done with the last K-tile's fragments
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            *reinterpret_cast<f32x4*>(lds + (wm * TM + mi * 32 + l31) * TS + wn * TN + ni * 32 + 8 * q + 4 * lhi) =
                                f32x4{acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
                __syncthreads();
                constexpr int CPR = BN / 4, RPP = NT / CPR, PASSES = BM / RPP;     // 16-B pieces per row, rows per pass
                const int c4 = tid % CPR, r0 = tid / CPR;
#pragma unroll 1
                for (int pb = 0; pb < PASSES; pb += 4) {
                    f32x4 pv[4], mv[4], vv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {                     // 12 x 16-B loads in flight per lane
                        const int64_t o = (m0 + r0 + (pb + u) * RPP) * g.ldc + n0 + 4 * c4;
                        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g.ad_p + o));
                        mv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g.ad_m + o));
                        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g.ad_v + o));
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int row = r0 + (pb + u) * RPP;
                        const int64_t o = (m0 + row) * g.ldc + n0 + 4 * c4;
                        const f32x4 gv = *reinterpret_cast<const f32x4*>(lds + row * TS + 4 * c4);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            mv[u][j] = mv[u][j] + omb1 * (gv[j] - mv[u][j]);
                            vv[u][j] = vv[u][j] + omb2 * (gv[j] * gv[j] - vv[u][j]);
                            pv[u][j] = pv[u][j] + (-lr * (mv[u][j] * ic1) / (sqrtf(vv[u][j] * ic2) + eps));
                        }
                        __builtin_nontemporal_store(mv[u], reinterpret_cast<f32x4*>(g.ad_m + o));
                        __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4*>(g.ad_v + o));
                        *reinterpret_cast<f32x4*>(g.ad_p + o) = pv[u];             // the next forward reads it
                        if (g.C != nullptr) *reinterpret_cast<f32x4*>(g.C + o) = gv;
                    }
                }
                return;
            }
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int64_t row = m0 + wm * TM + mi * 32 + l31;
                if (row >= g.M) continue;
                f32x4 pv[4], mv[4], vv[4];
                bool live[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {                      // 12 x 16-B loads in flight per lane
                    const int64_t col = n0 + wn * TN + ni * 32 + 8 * q + 4 * lhi;
                    live[q] = col < g.N;
                    const int64_t o = row * g.ldc + (live[q] ? col : 0);
                    pv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g.ad_p + o));
                    mv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g.ad_m + o));
                    vv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g.ad_v + o));
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!live[q]) continue;
                    const int64_t o = row * g.ldc + n0 + wn * TN + ni * 32 + 8 * q + 4 * lhi;
                    f32x4 gv;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float gi = acc[mi][ni][4 * q + j];
                        gv[j] = gi;
                        mv[q][j] = mv[q][j] + omb1 * (gi - mv[q][j]);
                        vv[q][j] = vv[q][j] + omb2 * (gi * gi - vv[q][j]);
                        pv[q][j] = pv[q][j] + (-lr * (mv[q][j] * ic1) / (sqrtf(vv[q][j] * ic2) + eps));
                    }
                    __builtin_nontemporal_store(mv[q], reinterpret_cast<f32x4*>(g.ad_m + o));
                    __builtin_nontemporal_store(vv[q], reinterpret_cast<f32x4*>(g.ad_v + o));
                    *reinterpret_cast<f32x4*>(g.ad_p + o) = pv[q];                 // the next forward reads it
                    if (g.C != nullptr) *reinterpret_cast<f32x4*>(g.C + o) = gv;
                }
            }
        return;
    }
    {
        float* const dst = g.splits > 1 ? g.ws + (int64_t)blockIdx.z * g.M * g.N : g.C;
        const int64_t ldd = g.splits > 1 ? g.N : g.ldc;
        const bool vec_c = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && ldd % 4 == 0;
        constexpr int TS = BN + 4;
        if constexpr (BM * TS <= 2 * (A_ELEMS + B_ELEMS) && (BN / 4) <= NT && NT % (BN / 4) == 0) {
            // interior tiles leave through LDS too: row-major 16-B stores, a wave instruction covering whole 256-B tile rows
            // instead of 32 rows x 32 B (measured, 128x64 tiles: dW 4096x4096x512 103-105 -> 108-109 TFLOP/s, the M = 512
            // products +1-3 %)
            if (g.staged_c && vec_c && m0 + BM <= g.M && n0 + BN <= g.N) {
                __syncthreads();
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            *reinterpret_cast<f32x4*>(lds + (wm * TM + mi * 32 + l31) * TS + wn * TN + ni * 32 + 8 * q + 4 * lhi) =
                                f32x4{acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
                __syncthreads();
                constexpr int CPR = BN / 4, RPP = NT / CPR, PASSES = BM / RPP;
                const int c4 = tid % CPR, r0 = tid / CPR;
#pragma unroll
                for (int pb = 0; pb < PASSES; ++pb) {
                    const int row = r0 + pb * RPP;
                    f32x4 gv = *reinterpret_cast<const f32x4*>(lds + row * TS + 4 * c4);
                    if (g.splits == 1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) gv[j] = apply_epilogue(g, gv[j], m0 + row, n0 + 4 * c4 + j);
                    }
                    *reinterpret_cast<f32x4*>(dst + (m0 + row) * ldd + n0 + 4 * c4) = gv;
                }
                return;
            }
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int64_t row = m0 + wm * TM + mi * 32 + l31;
                if (row >= g.M) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t col = n0 + wn * TN + ni * 32 + 8 * q + 4 * lhi;
                    if (col >= g.N) continue;
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] = acc[mi][ni][4 * q + j];
                        if (g.splits == 1 && col + j < g.N) v[j] = apply_epilogue(g, v[j], row, col + j);
                    }
                    if (vec_c && col + 3 < g.N) {
                        *reinterpret_cast<float4*>(dst + row * ldd + col) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (col + j < g.N) dst[row * ldd + col + j] = v[j];
                    }
                }
            }
    }
    TNN_GEMM_STAMP_ACKED(g.trace, (size_t)blockIdx.x, 8, g.trace ? ~(size_t)0 : 0, 3);
#undef TNN_TRACE
}

__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs g) {
    int64_t total = g.M * g.N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int z = 0; z < g.splits; ++z) s += g.ws[(int64_t)z * total + i];
        int64_t row = i / g.N, col = i - row * g.N;
        g.C[row * g.ldc + col] = apply_epilogue(g, s, row, col);
    }
}
