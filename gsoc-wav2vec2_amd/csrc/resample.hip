// Polyphase resampling with a rational ratio (w2v2_resample, w2v2_resample_design).
//
// Definition (include/w2v2.h; tests/resample_reference.py is the same in fp64 numpy).  For output n of a segment x[0, len), zero
// outside, with 64-bit integers q = floor(n M / L), r = (n M) mod L:
//     out[n] = sum_{t < K} table[r][t] x[q - lead + t]
// as ONE fp32 chain in ascending t over all K taps, pads included: acc = table[r][0] * x[.], then acc = fmaf(table[r][t], x[.], acc).
// Every output is such a chain whatever block or lane computes it, so the bits depend on the segment, the table and n alone; the
// product that starts the chain (not an fmaf onto +0) lets the copy filter [[1.0]] return -0.0 as -0.0.
//
// Structure.  One launch; a block owns `tile` consecutive outputs of one segment (W2V2_RESAMPLE_TILE, fewer for a filter whose
// input span per tile would not fit the LDS) and finds its segment by bisection of the segments' first tiles.
//   1. the tile's input span, floor(n0 M / L) - lead .. + (tile - 1) M / L + K, goes to LDS once with coalesced 4-byte loads (a
//      segment may start at any float), zero outside [0, len): no neighbour's sample is ever read.
//   2. lanes are mapped to outputs PHASE-MAJOR: the tile's outputs sorted by (i mod L, i div L).  Outputs L apart share the table
//      row r, so a wave reads one row (L < tile / 64) or a few rows as broadcasts, each walked in ascending t -- instead of 64 rows
//      per tap for consecutive outputs (row-major table, r stepping by M mod L).  Their input windows lie exactly M apart in LDS:
//      conflict-free for odd M, (M & -M)-way for even M.
//   3. results go to LDS at their output index and leave as coalesced stores.
// A filter whose span cannot be staged even for 64 outputs (K or M / L in the tens of thousands) takes the direct path of the same
// kernel: consecutive outputs per lane, samples read from global memory with the same bounds; the same chain, the same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace w2v2 {
namespace {

constexpr int RS_NT = 256;
constexpr int RS_LDS_FLOATS = 16384;       // 64 KB of dynamic LDS at the most: a tile's input span and its outputs
constexpr int RS_MIN_TILE = 64;            // a staged tile has at least this many outputs

struct RsFilt {
    const float* table;
    int32_t L, M, K, lead;
    int32_t qM, rM;        // M = qM L + rM
    int32_t tile;          // outputs per block
    int32_t staged;        // the input span of a tile fits the LDS
};

struct RsSeg {
    int64_t in0, out0, out_len;
    int64_t tile0;         // first block of the segment
    int32_t in_len, filt;
};

struct RsArgs {
    const float* in;
    float* out;
    const RsFilt* filts;
    const RsSeg* segs;
    int32_t nseg;
    int32_t linear;        // tuning build only (W2V2_RESAMPLE_LINEAR=1): lane k takes output k, the mapping the phase-major one replaced
};
// LDS: the tile's outputs in [0, W2V2_RESAMPLE_TILE), behind them the input span (at most RS_LDS_FLOATS in all)

// floats of input that `tile` consecutive outputs can span, whatever the phase of the first
inline int64_t tile_span(const RsFilt& f, int64_t tile) {
    return (tile - 1) * f.qM + ((int64_t)(f.L - 1) + (tile - 1) * f.rM) / f.L + f.K;
}

__global__ __launch_bounds__(RS_NT) void resample_kernel(RsArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    int lo = 0, hi = a.nseg - 1;               // the last segment whose first tile is not behind b (uniform over the block)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.segs[mid].tile0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const RsSeg sg = a.segs[lo];
    const RsFilt f = a.filts[sg.filt];
    const int64_t n0 = (b - sg.tile0) * f.tile;
    const int cnt = (int)min((int64_t)f.tile, sg.out_len - n0);
    const int64_t nM = n0 * f.M;
    const int64_t q0 = nM / f.L;
    const int r0 = (int)(nM - q0 * f.L);
    const float* __restrict__ x = a.in + sg.in0;
    float* __restrict__ y = a.out + sg.out0 + n0;
    const int K = f.K;

    if (!f.staged) {
        for (int i = tid; i < cnt; i += RS_NT) {
            const int64_t m = nM + (int64_t)i * f.M;
            const int64_t q = m / f.L;
            const float* __restrict__ row = f.table + (m - q * f.L) * K;
            const int64_t g0 = q - f.lead;
            float acc = row[0] * ((g0 >= 0 && g0 < sg.in_len) ? x[g0] : 0.0f);
            for (int t = 1; t < K; ++t) {
                const int64_t g = g0 + t;
                acc = fmaf(row[t], (g >= 0 && g < sg.in_len) ? x[g] : 0.0f, acc);
            }
            y[i] = acc;
        }
        return;
    }

    // 1. the span [first, first + span) of the segment, zero outside [0, in_len)
    float* ys = lds;
    float* xl = lds + W2V2_RESAMPLE_TILE;
    const int64_t first = q0 - f.lead;
    const int span = (int)((int64_t)(cnt - 1) * f.qM + ((int64_t)r0 + (int64_t)(cnt - 1) * f.rM) / f.L) + K;
    for (int i = tid; i < span; i += RS_NT) {
        const int64_t g = first + i;
        xl[i] = (g >= 0 && g < sg.in_len) ? x[g] : 0.0f;
    }
    __syncthreads();
    // 2. phase-major: residues below `rem` have base + 1 outputs in the tile, the others base
    const int L = f.L;
    const int base = cnt / L, rem = cnt - base * L, split = rem * (base + 1);
    for (int k = tid; k < cnt; k += RS_NT) {
        int rho, j;
        if (k < split) {
            rho = k / (base + 1);
            j = k - rho * (base + 1);
        } else {
            const int d = (k - split) / base;
            rho = rem + d;
            j = (k - split) - d * base;
        }
        const int i = a.linear ? k : rho + j * L;
        const unsigned w = (unsigned)r0 + (unsigned)i * (unsigned)f.rM;      // below 2^12 + 2^11 2^12
        const unsigned dq = w / (unsigned)L;
        const float* __restrict__ row = f.table + (int64_t)(w - dq * (unsigned)L) * K;
        const float* xs = xl + (i * f.qM + (int)dq);
        float acc = row[0] * xs[0];
#pragma unroll 4
        for (int t = 1; t < K; ++t) acc = fmaf(row[t], xs[t], acc);
        ys[i] = acc;
    }
    __syncthreads();
    // 3.
    for (int i = tid; i < cnt; i += RS_NT) y[i] = ys[i];
}

// I0(x), the modified Bessel function of the first kind and order zero: its power series, sum_k ((x / 2)^k / k!)^2
double bessel_i0(double x) {
    const double y = x * x / 4.0;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

}  // namespace

int64_t resample_length(int64_t len, int L, int M) {
    if (len < 0 || L < 1 || M < 1) return -1;
    const __int128 v = ((__int128)len * L + (M - 1)) / M;
    return v > (__int128)INT64_MAX ? -1 : (int64_t)v;
}

int resample_design(int rate_in, int rate_out, int zeros, double rolloff, double beta, int32_t* L_out, int32_t* M_out, int32_t* K_out,
                    int32_t* lead_out, float* table, int64_t table_capacity) {
    W2V2_REQUIRE(L_out && M_out && K_out && lead_out, "resample_design: null argument (L, M, K or lead)");
    W2V2_REQUIRE(rate_in >= 1 && rate_out >= 1, "resample_design: rates %d -> %d (need positive rates)", rate_in, rate_out);
    W2V2_REQUIRE(zeros >= 1, "resample_design: zeros = %d (need at least one)", zeros);
    W2V2_REQUIRE(rolloff > 0.0 && rolloff <= 1.0, "resample_design: rolloff = %g outside (0, 1]", rolloff);
    W2V2_REQUIRE(std::isfinite(beta) && beta >= 0.0, "resample_design: beta = %g (need a finite value >= 0)", beta);
    int g = rate_in, h = rate_out;
    while (h) {
        const int t = g % h;
        g = h;
        h = t;
    }
    const int M = rate_in / g, L = rate_out / g;
    *L_out = L;
    *M_out = M;
    if (L == M) {
        *K_out = 1;
        *lead_out = 0;
        if (table) {
            W2V2_REQUIRE(table_capacity >= 1, "resample_design: table_capacity = %lld floats, the table has 1", (long long)table_capacity);
            table[0] = 1.0f;
        }
        return W2V2_OK;
    }
    const double fc = (double)std::min(L, M) * rolloff / (double)M;
    const double width = std::ceil((double)zeros / fc);
    W2V2_REQUIRE(width < 1073741824.0, "resample_design: %d -> %d needs %.0f taps per output", rate_in, rate_out, 2.0 * width);
    const int K = 2 * (int)width, lead = (int)width - 1;
    *K_out = K;
    *lead_out = lead;
    if (!table) return W2V2_OK;
    W2V2_REQUIRE(table_capacity >= (int64_t)L * K, "resample_design: table_capacity = %lld floats, the table has %lld", (long long)table_capacity,
                 (long long)L * K);
    const double pi = 3.14159265358979323846, i0_beta = bessel_i0(beta);
    for (int r = 0; r < L; ++r)
        for (int t = 0; t < K; ++t) {
            const double u = (double)(t - lead) - (double)r / (double)L;
            const double s = u * fc;
            double v = 0.0;
            if (std::fabs(s) < (double)zeros) {
                const double a = pi * s, sw = s / (double)zeros;
                const double sinc = s == 0.0 ? 1.0 : std::sin(a) / a;
                v = fc * sinc * bessel_i0(beta * std::sqrt(1.0 - sw * sw)) / i0_beta;
            }
            table[(int64_t)r * K + t] = (float)v;
        }
    return W2V2_OK;
}

int launch_resample(const float* in, int n, const int64_t* in0, const int64_t* in_len, const int32_t* filter_of,
                    const w2v2_resample_filter* filters, int n_filters, float* out, const int64_t* out0, hipStream_t s) {
    W2V2_REQUIRE(in && in0 && in_len && filters && out && out0, "resample: null argument (in_dev, in0_host, in_len_host, filters, out_dev or out0_host)");
    W2V2_REQUIRE(n >= 1, "resample: n = %d segments (need at least one)", n);
    W2V2_REQUIRE(n_filters >= 1, "resample: n_filters = %d (need at least one)", n_filters);
    std::vector<RsFilt> filts((size_t)n_filters);
    int x_floats = 0;
    for (int k = 0; k < n_filters; ++k) {
        const w2v2_resample_filter& u = filters[k];
        W2V2_REQUIRE(u.table_dev, "resample: filters[%d].table_dev is null", k);
        W2V2_REQUIRE(u.L >= 1 && u.L <= W2V2_RESAMPLE_MAX_L, "resample: filters[%d].L = %d outside [1, %d]", k, u.L, W2V2_RESAMPLE_MAX_L);
        W2V2_REQUIRE(u.M >= 1, "resample: filters[%d].M = %d (need at least 1)", k, u.M);
        W2V2_REQUIRE(u.K >= 1, "resample: filters[%d].K = %d (need at least 1)", k, u.K);
        W2V2_REQUIRE((int64_t)u.L * u.K <= W2V2_RESAMPLE_MAX_TABLE, "resample: filters[%d]: L K = %lld table entries, at most %d", k,
                     (long long)u.L * u.K, W2V2_RESAMPLE_MAX_TABLE);
        W2V2_REQUIRE(u.lead >= 0 && u.lead < u.K, "resample: filters[%d].lead = %d outside [0, K = %d)", k, u.lead, u.K);
        RsFilt& f = filts[k];
        f = RsFilt{u.table_dev, u.L, u.M, u.K, u.lead, u.M / u.L, u.M % u.L, W2V2_RESAMPLE_TILE, 0};
        // the most outputs per block, up to the tile, whose input span fits the LDS behind the outputs (tile_span grows with the tile)
        int64_t fit = 0;
        for (int64_t a = 1, b = W2V2_RESAMPLE_TILE; a <= b;) {
            const int64_t mid = (a + b) / 2;
            if (tile_span(f, mid) + W2V2_RESAMPLE_TILE <= RS_LDS_FLOATS) {
                fit = mid;
                a = mid + 1;
            } else {
                b = mid - 1;
            }
        }
        if (fit >= RS_MIN_TILE) {
            f.tile = (int32_t)fit;
            f.staged = 1;
            x_floats = std::max(x_floats, (int)tile_span(f, fit));
        }
    }
    std::vector<RsSeg> segs((size_t)n);
    int64_t tiles = 0;
    double taps = 0.0, floats = 0.0;
    for (int i = 0; i < n; ++i) {
        W2V2_REQUIRE(in_len[i] >= 1 && in_len[i] < ((int64_t)1 << 31), "resample: in_len_host[%d] = %lld outside [1, 2^31)", i, (long long)in_len[i]);
        W2V2_REQUIRE(in0[i] >= 0, "resample: in0_host[%d] = %lld is negative", i, (long long)in0[i]);
        W2V2_REQUIRE(out0[i] >= 0, "resample: out0_host[%d] = %lld is negative", i, (long long)out0[i]);
        const int k = filter_of ? filter_of[i] : 0;
        W2V2_REQUIRE(k >= 0 && k < n_filters, "resample: filter_of_host[%d] = %d outside [0, n_filters = %d)", i, k, n_filters);
        const RsFilt& f = filts[k];
        const int64_t out_len = resample_length(in_len[i], f.L, f.M);
        segs[i] = RsSeg{in0[i], out0[i], out_len, tiles, (int32_t)in_len[i], k};
        tiles += (out_len + f.tile - 1) / f.tile;
        W2V2_REQUIRE(tiles < ((int64_t)1 << 31), "resample: more than 2^31 - 1 tiles of %d outputs", W2V2_RESAMPLE_TILE);
        taps += (double)out_len * f.K;
        floats += (double)in_len[i] + (double)out_len;
    }
    // workspace: the filters | the segments
    const size_t filt_bytes = ((size_t)n_filters * sizeof(RsFilt) + 15) & ~(size_t)15, seg_bytes = (size_t)n * sizeof(RsSeg);
    void* raw = nullptr;
    if (int e = stream_scratch(SCRATCH_RESAMPLE, s, filt_bytes + seg_bytes, &raw)) return e;
    if (int e = staged_upload(SCRATCH_RESAMPLE, s, raw,
                              {{filts.data(), (size_t)n_filters * sizeof(RsFilt), 0}, {segs.data(), seg_bytes, filt_bytes}}, (size_t)16 << 10))
        return e;
    RsArgs a{};
    a.in = in;
    a.out = out;
    a.filts = reinterpret_cast<const RsFilt*>(raw);
    a.segs = reinterpret_cast<const RsSeg*>(static_cast<char*>(raw) + filt_bytes);
    a.nseg = n;
    a.linear = tune_int("W2V2_RESAMPLE_LINEAR", 0);
    // (work for the profile: one fused multiply-add per tap; every sample read and every output written once)
    ProfScope ps(nullptr, FAM_MISC, 2.0 * taps, 4.0 * floats, s);
    W2V2_LAUNCH(resample_kernel, dim3((unsigned)tiles), dim3(RS_NT), (size_t)(W2V2_RESAMPLE_TILE + x_floats) * sizeof(float), s, a);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
