// fp32 GEMM with an NS-stage LDS ring and an optional persistent tile loop (the forward's wide and 128 x 128 shapes).
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
#include "common.h"
#include "gemm_epilogue.h"
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
    int M, N, K, act;
    int tiles_m, tiles_n, nbatch;
    int gm;          // grouped tile order (common.h::grouped_tile); 0 = linear order
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
template <int WM, int WN, int BKT, int BM, int BN, int NS>
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

    const int nwg = g.tiles_m * g.tiles_n, total = nwg * g.nbatch, G = gridDim.x;
    const int ntl = (total - (int)blockIdx.x + G - 1) / G;      // tiles of this block (the grid never exceeds the tile count)
    const int nk = g.K / BKT, nsteps = ntl * nk;
    // i-th tile of this block -> (batch, first row, first column).  XCD-aware order over the flat tile range: G is a multiple
    // of 8 (or the tile count), so tile v runs on XCD v % 8 as blockIdx.x does; each XCD owns a contiguous run, N fastest.
    auto tile_of = [&](int i, int& z, int& m0, int& n0) {
        const int v = (int)blockIdx.x + i * G;
        const int q = total >> 3, r = total & 7, xcd = v & 7, idx = v >> 3;
        int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        z = t / nwg;
        t -= z * nwg;
        int tm = t / g.tiles_n, tn = t % g.tiles_n;
        if (g.gm > 0) grouped_tile(t, g.tiles_m, g.tiles_n, g.gm, tm, tn);
        m0 = tm * BM;
        n0 = tn * BN;
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
        int z, m0, n0;
        tile_of(ci, z, m0, n0);
        const int64_t tile_off = (int64_t)z * g.strideC + (int64_t)(m0 + wm * WTM) * g.ldc + (n0 + wn * WTN);
        // (the epilogue's loop-invariant switches are laundered through asm: otherwise the compiler unswitches the tile loop on
        //  them, and hoists the per-element store offsets, which depend on ldc and the lane only, out of it: 64+ registers held
        //  live across the K loop, 255 VGPRs and scratch at 256 x 128)
        int act = g.act, ldc = (int)g.ldc, eli = li, elh = lh;
        const float* res = g.residual;
        const float* bias = g.bias;
        asm volatile("" : "+s"(act), "+s"(res), "+s"(bias), "+s"(ldc), "+v"(eli), "+v"(elh));
        __builtin_amdgcn_s_setprio(0);
        gemm_epilogue<MT, NTL, false>(acc, g.C + tile_off, nullptr, res ? res + tile_off : nullptr, bias ? bias + (n0 + wn * WTN) : nullptr,
                                     ldc, g.M - (m0 + wm * WTM), g.N - (n0 + wn * WTN), act, eli, elh);
        __builtin_amdgcn_s_setprio(1);
    }
    __builtin_amdgcn_s_setprio(0);
}

template <int WM, int WN, int BKT, int BM, int BN, int NS>
int launch_ring(GemmRingArgs& g, bool persist, hipStream_t s) {
    using R_ = RingCfg<WM, WN, BKT, BM, BN, NS>;
    static_assert(2 * R_::LDS <= 160 * 1024, "two blocks per CU");
    g.tiles_m = (g.M + BM - 1) / BM;
    g.tiles_n = (g.N + BN - 1) / BN;
    const int64_t total = (int64_t)g.tiles_m * g.tiles_n * g.nbatch;
    W2V2_REQUIRE(total < (1ll << 31), "gemm ring: %lld tiles", (long long)total);
    int grid = (int)total;
    if (persist) {
        int dev = 0, cus = 0;
        W2V2_HIP_CHECK(hipGetDevice(&dev));
        W2V2_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int resident = (2 * cus) & ~7;            // two blocks per CU, a multiple of the 8 XCDs
        if (resident >= 8 && total > resident) grid = resident;
    }
    // (tiles an XCD has in flight, as counted for the gemm_f32_dma_kernel instance of the same tile: same tile order)
    g.gm = g.nbatch == 1 ? tile_group_rows(g.tiles_m, g.tiles_n, (int64_t)BM * g.K * 4, BM == 256 ? 96 : 64) : 0;
    static std::atomic<bool> attr_set{false};
    if (!attr_set) {
        W2V2_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_ring_kernel<WM, WN, BKT, BM, BN, NS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, R_::LDS));
        attr_set = true;
    }
    W2V2_LAUNCH((gemm_f32_ring_kernel<WM, WN, BKT, BM, BN, NS>), dim3(grid), dim3(WM * WN * 64), R_::LDS, s, g);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace

bool gemm_f32_ring_ok(int tile, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, int64_t strideB,
                      int M, int N, int K) {
    const int BM = tile == 0 ? 256 : 128, BKT = 16;
    const bool align = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 && lda % 4 == 0 &&
                       ldb % 4 == 0 && strideA % 4 == 0 && strideB % 4 == 0;
    // per-lane DMA offsets are 32-bit byte offsets from the tile's row / column base
    return align && K % BKT == 0 && N % 4 == 0 && N >= 4 && (int64_t)BM * lda * 4 < (1ll << 31) &&
           (int64_t)BKT * ldb * 4 < (1ll << 31) && M > 0;
}

int launch_gemm_f32_ring(int tile, bool persist, const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb,
                         int64_t strideB, float* C, int64_t ldc, int64_t strideC, const float* bias, const float* residual, int M,
                         int N, int K, int nbatch, int act, hipStream_t s) {
    W2V2_REQUIRE(tile == 0 || tile == 1, "gemm ring: tile %d", tile);
    W2V2_REQUIRE(gemm_f32_ring_ok(tile, A, lda, strideA, B, ldb, strideB, M, N, K), "gemm ring: unsupported shape M=%d N=%d K=%d", M, N, K);
    GemmRingArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.residual = residual;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.strideA = strideA; g.strideB = strideB; g.strideC = strideC;
    g.M = M; g.N = N; g.K = K; g.act = act; g.nbatch = nbatch;
    if (tile == 0) return launch_ring<4, 2, 16, 256, 128, 3>(g, persist, s);      // 72 KiB: two blocks per CU
    return launch_ring<2, 4, 16, 128, 128, 4>(g, persist, s);                     // 64 KiB
}

}  // namespace w2v2
