// fp32 GEMM with an NS-stage LDS ring and an optional persistent tile loop (the forward's wide, 128 x 128 and 64 x 64 shapes).
//
// Same tiles, wave grid, swizzled LDS images and MFMA loop as gemm_f32_dma_kernel (gemm_f32.hip); what differs is the
// pipeline around them:
//   * the K tiles stream HBM/L2 -> LDS through NS ring stages (LDS-DMA issued as asm with a scalar base, so the compiler
//     inserts no wait of its own for them), NS - 1 K tiles ahead of the MFMAs instead of one;
//   * the wait before each block barrier is counted: vmcnt((NS - 2) x pieces per K tile) retires only the tile needed next,
//     the younger tiles stay in flight across the barrier (the double buffer's __syncthreads drains to vmcnt(0));
//   * a block may own several output tiles (grid of at most two blocks per CU, tiles v = blockIdx.x + i x gridDim.x): the
//     K tiles of all of them are ONE stream, so the next tile's first NS - 1 K tiles are in flight while this tile's
//     epilogue runs, and a block pays its prologue once;
//   * s_setprio(1) over the K loop: a block's MFMA waves outrank the other block's epilogue on the SIMD.
// Every output element consumes the same k pairs in the same order ({k, k+4} in each 8-wide block, k blocks ascending)
// from a zeroed accumulator, and the epilogue is gemm_epilogue: results are bit-identical to gemm_f32_dma_kernel.
// The epilogue's form (bias, exact GELU, residual) is a template argument: one instance per form the models use (ring_form below);
// any other combination, tanh GELU included, stays on gemm_f32_dma_kernel, whose epilogue takes its switches at run time.
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_f32_route.h"
#include "gemm_sw_common.h"

namespace w2v2 {

namespace {

struct GemmRingArgs {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    const float* residual;
    int64_t lda, ldb, ldc, strideA, strideB, strideC;
    int M, N, K;
    int tiles_m, tiles_n, nbatch;
    int gm;          // grouped tile order (common.h::grouped_tile); 0 = linear order
    int total;       // tiles of this launch: tiles_m x tiles_n x nbatch, or a prefix of that order (the split launch below)
    int first;       // QUAD: first tile of the (2 BM) x (2 BN) grid's order that this launch takes, as four BM x BN tiles each
};

template <int WM, int WN, int BKT, int BM, int BN, int NS>
struct RingCfg {
    static constexpr int STAGE = (BM * BKT + BKT * BN) * 4;   // bytes per ring stage
    static constexpr int LDS = NS * STAGE;
    static constexpr int NW = WM * WN;
    static constexpr int NPA = BM * BKT / 256, NPB = BKT * BN / 256;   // 1-KiB DMA pieces per K tile
    static constexpr int PPA = NPA / NW, PPB = NPB / NW;                // ... per wave
    static constexpr int P = PPA + PPB;                                 // vmcnt units one K tile adds per wave
    static_assert(NPA % NW == 0 && NPB % NW == 0, "every wave issues the same number of pieces (counted waits)");
    static_assert((NS - 2) * P <= 63, "vmcnt field");
};

// (waves_per_eu(4): two 8-wave blocks per CU need <= 128 VGPRs; the 256 x 128 instance otherwise takes 132 and one block per CU)
// QUAD: tiles_m x tiles_n is the grid of (2 BM) x (2 BN) tiles; this launch runs tiles first, first + 1, ... of ITS order, four
// BM x BN quarters each (the rest of an order whose first `first` tiles ran at the large tile; M and N are multiples of the large tile).
// BIAS / GELU / RES: the epilogue's form.  As run-time values they had to be laundered through asm against loop unswitching, which left
// both GELU arms and the residual path in every instance (256 x 128: two spilled VGPRs); as constants each instance holds its own path only.
template <int WM, int WN, int BKT, int BM, int BN, int NS, bool QUAD, bool BIAS, bool GELU, bool RES>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(4))) void gemm_f32_ring_kernel(GemmRingArgs g) {
    using R_ = RingCfg<WM, WN, BKT, BM, BN, NS>;
    constexpr int NW = R_::NW, PPA = R_::PPA, PPB = R_::PPB, P = R_::P, STAGE = R_::STAGE;
    constexpr int RPP = 256 / BKT;              // A rows per 1-KiB piece
    constexpr int SPR = BKT / 4;                // 16-B k-slots per A row
    constexpr int SW = BKT == 32 ? 1 : 2;       // swizzle: slot ^= (row >> SW) & (SPR - 1)  (= gemm_f32_dma_kernel)
    constexpr int WTM = BM / WM, WTN = BN / WN, MT = WTM / 32, NTL = WTN / 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform: DMA destinations are scalar)
    const int wm = wave / WN, wn = wave % WN, li = lane & 31, lh = lane >> 5;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)smem;

    const int nwg = g.tiles_m * g.tiles_n, total = g.total, G = gridDim.x;
    const int ntl = (total - (int)blockIdx.x + G - 1) / G;      // tiles of this block (the grid never exceeds the tile count)
    const int nk = g.K / BKT, nsteps = ntl * nk;
    // i-th tile of this block -> (batch, first row, first column).  XCD-aware order over the flat tile range: G is a multiple
    // of 8 (or the tile count), so tile v runs on XCD v % 8 as blockIdx.x does; each XCD owns a contiguous run, N fastest.
    auto tile_of = [&](int i, int& z, int& m0, int& n0) {
        const int v = (int)blockIdx.x + i * G;
        const int q = total >> 3, r = total & 7, xcd = v & 7, idx = v >> 3;
        int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        int sub = 0;
        if constexpr (QUAD) {
            sub = t & 3;
            t = g.first + (t >> 2);
        }
        z = t / nwg;
        t -= z * nwg;
        int tm = t / g.tiles_n, tn = t % g.tiles_n;
        if (g.gm > 0) grouped_tile(t, g.tiles_m, g.tiles_n, g.gm, tm, tn);
        m0 = tm * BM;
        n0 = tn * BN;
        if constexpr (QUAD) {
            m0 = 2 * m0 + (sub >> 1) * BM;
            n0 = 2 * n0 + (sub & 1) * BN;
        }
    };

    // ---- issue side: cursor (tile ii, K tile ikt, ring stage ist), wave-uniform bases, per-lane 32-bit byte offsets
    int ii = 0, ikt = 0, ist = 0;
    const unsigned char* baseA = nullptr;
    const unsigned char* baseB = nullptr;
    uint32_t offA[PPA], offB[PPB];
    auto uniform_ptr = [](const void* p) {
        const uint64_t v = reinterpret_cast<uint64_t>(p);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        return reinterpret_cast<const unsigned char*>(((uint64_t)hi << 32) | lo);
    };
    auto set_issue_tile = [&](int i) {
        int z, m0, n0;
        tile_of(i, z, m0, n0);
        baseA = uniform_ptr(g.A + (int64_t)z * g.strideA + (int64_t)m0 * g.lda);
        baseB = uniform_ptr(g.B + (int64_t)z * g.strideB + n0);
#pragma unroll
        for (int p = 0; p < PPA; ++p) {
            const int r = (wave + p * NW) * RPP + lane / SPR;       // A row inside the tile
            const int rr = m0 + r < g.M ? r : g.M - 1 - m0;          // clamp: loads stay in bounds, stores are guarded
            const int slot = (lane % SPR) ^ ((r >> SW) & (SPR - 1));
            offA[p] = (uint32_t)((int64_t)rr * g.lda * 4) + (uint32_t)slot * 16u;
        }
#pragma unroll
        for (int p = 0; p < PPB; ++p) {
            const int flat = (wave + p * NW) * 256 + lane * 4;      // lane-linear position inside the (BKT, BN) image
            const int br = flat / BN, c = flat % BN;
            const int cc = n0 + c < g.N ? c : g.N - 4 - n0;          // clamped columns feed accumulators never stored (N % 4 == 0)
            offB[p] = (uint32_t)((int64_t)br * g.ldb * 4) + (uint32_t)cc * 4u;
        }
    };
    auto issue_step = [&]() {
        const unsigned dst = lds0 + (unsigned)ist * STAGE;
        const unsigned char* a = baseA + (int64_t)ikt * BKT * 4;
        const unsigned char* b = baseB + (int64_t)ikt * BKT * g.ldb * 4;
#pragma unroll
        for (int p = 0; p < PPA; ++p) sw_dma(dst + (unsigned)(wave + p * NW) * 1024u, offA[p], a);
#pragma unroll
        for (int p = 0; p < PPB; ++p) sw_dma(dst + (unsigned)(BM * BKT * 4) + (unsigned)(wave + p * NW) * 1024u, offB[p], b);
        ist = ist + 1 == NS ? 0 : ist + 1;
        if (++ikt == nk) {
            ikt = 0;
            if (++ii < ntl) set_issue_tile(ii);
        }
    };

    // ---- compute side (fragment reads and MFMA order of gemm_f32_dma_kernel)
    f32x16 acc[MT][NTL];
    auto zero = [&]() {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NTL; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    };
    int a_row[MT], a_swz[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int i = wm * WTM + mt * 32 + li;
        a_row[mt] = i * BKT;
        a_swz[mt] = (i >> SW) & (SPR - 1);
    }
    auto compute = [&](int stage) {
        const float* As = smem + stage * (STAGE / 4);
        const float* Bs = As + BM * BKT + (4 * lh) * BN + wn * WTN + li;
#pragma unroll
        for (int kb = 0; kb < BKT / 8; ++kb) {
            f32x4 a[MT];
            float b[NTL][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                a[mt] = *reinterpret_cast<const f32x4*>(As + a_row[mt] + (((2 * kb + lh) ^ a_swz[mt]) << 2));
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
                for (int e = 0; e < 4; ++e) b[nt][e] = Bs[(kb * 8 + e) * BN + nt * 32];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NTL; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][e], b[nt][e], acc[mt][nt], 0, 0, 0);
        }
    };
    // all of this wave's DMA but the youngest n pieces has landed; then every wave's has (barrier).  The asm memory clobbers keep
    // the fragment reads on their side of the barrier (the s_barrier builtin alone does not order memory for the compiler).
    auto ring_barrier = [&](bool counted) {
        if (counted) sw_wait_vm<(NS - 2) * P>();
        else sw_wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    set_issue_tile(0);
    for (int p = 0; p < NS - 1 && p < nsteps; ++p) issue_step();
    ring_barrier(nsteps >= NS - 1);                     // K tile 0 (the NS - 2 younger ones may be in flight)
    __builtin_amdgcn_s_setprio(1);

    int s = 0, cst = 0;                                  // step of the stream, ring stage it reads
    for (int ci = 0; ci < ntl; ++ci) {
        zero();
        int z, m0, n0;      // (worked out in front of the K loop, under the DMA in flight: the epilogue starts without tile_of's divisions)
        tile_of(ci, z, m0, n0);
        for (int kt = 0; kt < nk; ++kt, ++s) {
            const bool more = s + NS - 1 < nsteps;
            if (more) issue_step();                      // into the stage read at step s - 1 (every wave passed the barrier since)
            __builtin_amdgcn_sched_barrier(0);
            compute(cst);
            __builtin_amdgcn_sched_barrier(0);
            ring_barrier(more);                          // K tile s + 1 has landed; every wave is done reading stage cst
            cst = cst + 1 == NS ? 0 : cst + 1;
        }
        // epilogue of tile ci, with the next tile's first K tiles in flight: bias -> activation -> + residual -> store
        const int64_t tile_off = (int64_t)z * g.strideC + (int64_t)(m0 + wm * WTM) * g.ldc + (n0 + wn * WTN);
        // (ldc and the lane coordinates are laundered through asm: otherwise the compiler hoists the per-element store offsets, which
        //  depend on them only, out of the tile loop: 64+ registers held live across the K loop, 255 VGPRs and scratch at 256 x 128)
        int ldc = (int)g.ldc, eli = li, elh = lh;
        asm volatile("" : "+s"(ldc), "+v"(eli), "+v"(elh));
        __builtin_amdgcn_s_setprio(0);
        gemm_epilogue<MT, NTL, false, RES && MT * NTL <= 2>(acc, g.C + tile_off, nullptr, RES ? g.residual + tile_off : nullptr, BIAS ? g.bias + (n0 + wn * WTN) : nullptr,
                                     ldc, g.M - (m0 + wm * WTM), g.N - (n0 + wn * WTN), GELU ? 1 : 0, eli, elh);
        __builtin_amdgcn_s_setprio(1);
    }
    __builtin_amdgcn_s_setprio(0);
}

std::atomic<int64_t> g_ring_launches[4];      // 256 x 128, 128 x 128, 64 x 64, 64 x 64 quarters (gemm_f32_ring_launches)

// split launch (nbatch == 1, M and N multiples of the large tile): `first` tiles of the order, group height gm, run at the large tile
// (!QUAD: limit = first), the other tiles as quarters (QUAD).  first < 0: the whole problem.
template <int WM, int WN, int BKT, int BM, int BN, int NS, bool QUAD, bool BIAS, bool GELU, bool RES>
int launch_ring_form(GemmRingArgs& g, bool persist, hipStream_t s, int64_t first, int gm) {
    using R_ = RingCfg<WM, WN, BKT, BM, BN, NS>;
    static_assert(2 * R_::LDS <= 160 * 1024, "two blocks per CU");
    constexpr int TM = QUAD ? 2 * BM : BM, TN = QUAD ? 2 * BN : BN;
    g.tiles_m = (g.M + TM - 1) / TM;
    g.tiles_n = (g.N + TN - 1) / TN;
    int64_t total = (int64_t)g.tiles_m * g.tiles_n * g.nbatch;
    W2V2_REQUIRE(first < 0 || (first > 0 && first < total && g.nbatch == 1 && g.M % TM == 0 && g.N % TN == 0), "gemm ring: bad split");
    W2V2_REQUIRE(!QUAD || first > 0, "gemm ring: quarter tiles need a split");
    g.first = QUAD ? (int)first : 0;
    if (first > 0) total = QUAD ? 4 * (total - first) : first;
    W2V2_REQUIRE(total < (1ll << 31), "gemm ring: %lld tiles", (long long)total);
    g.total = (int)total;
    // blocks a CU holds: two of the 8-wave instances; the 4-wave 64 x 64 instance as many as its ring leaves LDS for (at most 4)
    constexpr int PER_CU = WM * WN == 8 ? 2 : 160 * 1024 / R_::LDS > 4 ? 4 : 160 * 1024 / R_::LDS;
    int grid = (int)total;
    if (persist) {
        int dev = 0, cus = 0;
        W2V2_HIP_CHECK(hipGetDevice(&dev));
        W2V2_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int resident = (PER_CU * cus) & ~7;       // a multiple of the 8 XCDs
        if (resident >= 8 && total > resident) grid = resident;
    }
    // (tiles an XCD has in flight, as counted for the gemm_f32_dma_kernel instance of the same tile: same tile order)
    g.gm = first > 0 ? gm : g.nbatch == 1 ? tile_group_rows(g.tiles_m, g.tiles_n, (int64_t)BM * g.K * 4, BM == 256 ? 96 : 32 * PER_CU) : 0;
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        W2V2_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_ring_kernel<WM, WN, BKT, BM, BN, NS, QUAD, BIAS, GELU, RES>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, R_::LDS));
        attr_set = true;
    }
    W2V2_LAUNCH((gemm_f32_ring_kernel<WM, WN, BKT, BM, BN, NS, QUAD, BIAS, GELU, RES>), dim3(grid), dim3(WM * WN * 64), R_::LDS, s, g);
    W2V2_HIP_CHECK(hipGetLastError());
    g_ring_launches[QUAD ? 3 : BM == 256 ? 0 : BM == 128 ? 1 : 2].fetch_add(1, std::memory_order_relaxed);
    return W2V2_OK;
}

// one instance per epilogue form (gemm_f32_route.h: gemm_f32_ring_form); the router keeps every other form on gemm_f32_dma_kernel
template <int WM, int WN, int BKT, int BM, int BN, int NS, bool QUAD = false>
int launch_ring(GemmRingArgs& g, int act, bool persist, hipStream_t s, int64_t first = -1, int gm = 0) {
    switch (gemm_f32_ring_form(g.bias != nullptr, g.residual != nullptr, act)) {
        case 0: return launch_ring_form<WM, WN, BKT, BM, BN, NS, QUAD, false, false, false>(g, persist, s, first, gm);
        case 1: return launch_ring_form<WM, WN, BKT, BM, BN, NS, QUAD, true, false, false>(g, persist, s, first, gm);
        case 2: return launch_ring_form<WM, WN, BKT, BM, BN, NS, QUAD, true, true, false>(g, persist, s, first, gm);
        case 3: return launch_ring_form<WM, WN, BKT, BM, BN, NS, QUAD, true, false, true>(g, persist, s, first, gm);
        case 4: return launch_ring_form<WM, WN, BKT, BM, BN, NS, QUAD, false, false, true>(g, persist, s, first, gm);
        case 5: return launch_ring_form<WM, WN, BKT, BM, BN, NS, QUAD, false, true, false>(g, persist, s, first, gm);
    }
    W2V2_REQUIRE(false, "gemm ring: no instance for this epilogue (bias %d, residual %d, act %d)", g.bias != nullptr, g.residual != nullptr, act);
    return W2V2_OK;
}

}  // namespace

void gemm_f32_ring_launches(int64_t* counts) {
    for (int i = 0; i < 4; ++i) counts[i] = g_ring_launches[i].load(std::memory_order_relaxed);
}

bool gemm_f32_ring_ok(int tile, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, int64_t strideB,
                      int M, int N, int K) {
    const bool ab_aligned = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0;
    return gemm_f32_ring_shape_ok(tile, ab_aligned, lda, strideA, ldb, strideB, M, N, K);
}

int launch_gemm_f32_ring(int tile, bool persist, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb,
                         int64_t strideB, float* C, int64_t ldc, int64_t strideC, const float* bias, const float* residual, int M,
                         int N, int K, int nbatch, int act, hipStream_t s) {
    W2V2_REQUIRE(tile >= 0 && tile <= 2, "gemm ring: tile %d", tile);
    W2V2_REQUIRE(gemm_f32_ring_ok(tile, A, lda, strideA, B, ldb, strideB, M, N, K), "gemm ring: unsupported shape M=%d N=%d K=%d", M, N, K);
    GemmRingArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.residual = residual;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.strideA = strideA; g.strideB = strideB; g.strideC = strideC;
    g.M = M; g.N = N; g.K = K; g.nbatch = nbatch;
    if (tile == 0) return launch_ring<4, 2, 16, 256, 128, 3>(g, act, persist, s);      // 72 KiB: two blocks per CU
    if (tile == 1) return launch_ring<2, 4, 16, 128, 128, 4>(g, act, persist, s);      // 64 KiB
    // 64 x 64, four waves of 32 x 32 (the tail rows and the small problems).  48 KiB: three blocks per CU, so the 528 tail tiles of
    // N = 768 at B = 32 are all resident at once, as with the double buffer; the 64-KiB 32 x 4 ring runs them in two rounds and loses
    // (instances 16 x 4 / 5 / 6 and 32 x 4 measured and dropped: profiles/ring_tail_ab.md).
    return launch_ring<2, 2, 32, 64, 64, 3>(g, act, persist, s);
}

// One GEMM as two launches that split the 128 x 128 tile order (XCD runs, grouped rows) at `main_tiles`: the first main_tiles tiles on
// the 128 x 128 ring kernel, every later tile as four 64 x 64 quarters on the 64 x 64 one.  With main_tiles a multiple of the resident
// 128 x 128 slots and at most a quarter of them left over, both launches fill the CUs evenly: two 8-wave blocks per CU in whole rounds,
// then at most two 4-wave blocks per CU (whole tile ROWS for the second launch leave 528 tiles for 512 such places at N = 768, B = 32:
// sixteen CUs run three blocks and everything waits for them).  Needs M % 128 == 0 and N % 128 == 0: no quarter lies outside C.
int launch_gemm_f32_ring_split(bool persist, int64_t main_tiles, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                               int64_t ldc, const float* bias, const float* residual, int M, int N, int K, int act, hipStream_t s) {
    W2V2_REQUIRE(M % 128 == 0 && N % 128 == 0 && gemm_f32_ring_ok(1, A, lda, 0, B, ldb, 0, M, N, K) && gemm_f32_ring_ok(2, A, lda, 0, B, ldb, 0, M, N, K),
                 "gemm ring split: unsupported shape M=%d N=%d K=%d", M, N, K);
    GemmRingArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.residual = residual;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.strideA = 0; g.strideB = 0; g.strideC = 0;
    g.M = M; g.N = N; g.K = K; g.nbatch = 1;
    const int gm = tile_group_rows(M / 128, N / 128, (int64_t)128 * K * 4, 64);
    if (int e = launch_ring<2, 4, 16, 128, 128, 4>(g, act, persist, s, main_tiles, gm)) return e;
    return launch_ring<2, 2, 32, 64, 64, 3, true>(g, act, false, s, main_tiles, gm);
}

}  // namespace w2v2
