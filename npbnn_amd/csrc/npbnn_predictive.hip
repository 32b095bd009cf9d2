// The posterior predictive distribution of a regression (include/npbnn_hip.h: npbnn_op_mixture, npbnn_predict_sets_predictive): its
// quantiles, its mean and its continuous ranked probability score.  A cell - one (row, target) pair - has S components mu_s, sigma_s,
// and its predictive distribution is the mixture (1/S) sum_s N(mu_s, sigma_s^2).  All arithmetic is float64:
//   F(x)       = (1/S) sum_s Phi((x - mu_s) / sigma_s),  Phi(u) = 0.5 erfc(-u / sqrt 2)
//   quantile_p = the x with F(x) = p (F is continuous and strictly increasing)
//   mean       = K + (1/S) sum_s (mu_s - K), K = mu_1 (as npbnn_predict_sets_calibration forms it)
//   A(m, v)    = 2 sqrt(v) phi(m / sqrt v) + m erf(m / sqrt(2 v)) = E|N(m, v)|, written with erf so that both terms are >= 0
//   crps(y)    = (1/S) sum_s A(y - mu_s, sigma_s^2) - (1/(2 S^2)) [sum_s 2 sigma_s / sqrt(pi) + 2 sum_{s<t} A(mu_s - mu_t, sigma_s^2 + sigma_t^2)]
// The reference has no counterpart: its summary code takes calcHPD of the means (np_bnn/BNN_plot.py:73-75), which leaves the noise out.
//
// Both kernels are stack column kernels (npbnn_stack.hip.h: the tile rule of npbnn_stack_plan.h, the loader, the wave reductions
// and the launch they share with hpd_kernel and convergence_kernel): a workgroup takes a tile of adjacent cells into LDS - mu in
// the input's type, and sigma beside it when it has mu's type and layout; a per-sample float64 sigma [S][T] is small, shared by every
// cell of a target, and is read where it lies.  A single cell that does not fit the LDS (float64 mu and sigma at S = 16384) is not
// staged: every pass reads it from global memory.  One wave works on one cell at a time, its 64 lanes stride over S (over the pairs
// s < t in row-major order for the pair term), each lane adds its terms one after the other and a fixed xor butterfly leaves the
// same bits of the sum in every lane: every decision of the root search is wave-uniform, and the bits of a cell's result depend on
// the cell's values and on S alone - not on the tile, the grid or how the replay grouped the sets.  No atomics but the flag word.
//
// mixture_quantile_kernel: per probability, the bracket [min_s (mu_s + sigma_s z_p), max_s (...)] holds the root in exact arithmetic
// (z_p from the host: Newton on libm's erfc); the kernel evaluates both ends and widens by doubling while an end is on the wrong
// side.  Then safeguarded Newton steps - F and the density from one pass over S - with a bisection step whenever the Newton step
// leaves the bracket, until the bracket cannot narrow, a point meets the probability exactly, or kMixMaxSteps passes are spent.  For
// p > 0.5 the search runs on the upper tail, sum erfc(+u) against 1 - p (exact for p >= 0.5), so a tail keeps its relative precision.
// The end of the last bracket with the smaller residual is returned.
//
// Floating-point contraction (the rule of npbnn_fold.hip.h): this unit's definitions are float64 sums of products whose bits a test
// compares against a restatement, so contraction is switched off for the whole unit after the includes; the headers above it hold no
// product that feeds a sum (npbnn_stack.hip.h and npbnn_sets.hip.h say so of themselves) and are not touched by it.
#include "npbnn_stack.hip.h"

#include <cfloat>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace npbnn_api {

namespace {

constexpr int kMixMaxProbs = 16;
constexpr int kMixMaxSteps = 200;                  // passes of the root search (a CPU emulation of the scheme needed 77 at most)
constexpr int kMixMaxWiden = 128;                  // doublings of an end that is on the wrong side
constexpr double kMinTail = 1e-12;                 // min(p, 1 - p) at least
constexpr int kFlagBadSigma = 8;                   // (beside kFlagNaN: a mu that is not finite)

constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kInvSqrt2Pi = 0.39894228040143267794;
constexpr double kTwoOverSqrtPi = 1.12837916709551257390;

struct MixParams {
    const void* mu;           // cell c, sample s: mu[s * col_stride + cell_off(c)]
    const void* sg;           // sigma_cols == 0: sigma in mu's type at the same place
    const double* sg64;       // sigma_cols == T: [S][T], cell c reads column c % T
    long long n_cols, col_stride;
    int cells_per_row, row_pitch;      // cell_off(c) = (c / cells_per_row) * row_pitch + c % cells_per_row
    int S, sigma_cols, tile, log2tile;
    int n_probs;
    double p[kMixMaxProbs], z[kMixMaxProbs];
    const double* y;          // [n_cols] (CRPS)
    double* quantile;         // [n_probs][n_cols], or nullptr
    double* mean;             // [n_cols], or nullptr
    double* crps;             // [n_cols]
    int* flag;
};

__device__ inline long long cell_off(const MixParams& p, long long c) {
    return (c / p.cells_per_row) * p.row_pitch + c % p.cells_per_row;
}

// One cell's components: mu and sigma of sample s, from the LDS copy or from where they lie.
template <class V, bool SIG64>
struct Cell {
    const V* mu;
    const V* sg;
    const double* sg64;
    long long stride;         // between two samples of mu (and of a same-type sigma)
    int sg_stride;            // between two samples of sg64
    __device__ double m(int s) const { return (double)mu[s * stride]; }
    __device__ double sd(int s) const { return SIG64 ? sg64[(long long)s * sg_stride] : (double)sg[s * stride]; }
};

// The workgroup's tile into LDS (adjacent cells are contiguous within a row of the table): mu [tile][pitch], then sigma [tile][pitch]
// unless SIG64.  Every thread of the workgroup calls it.
template <class V, bool SIG64>
__device__ inline void stage_tile(const MixParams& p, V* sh, long long c0, int tc, int pitch) {
    load_stack_tile<SIG64 ? 1 : 2, false, false>(sh, static_cast<const V*>(p.mu), static_cast<const V*>(p.sg), p.col_stride, p.S, p.S, (V)0, p.tile,
                                                 p.log2tile, tc, pitch, [&p, c0](int c) { return cell_off(p, c0 + c); });
    __syncthreads();
}

// cell c0 + c of the tile
template <class V, bool SIG64, bool STAGED>
__device__ inline Cell<V, SIG64> cell_of(const MixParams& p, const V* sh, long long c0, int c, int pitch) {
    Cell<V, SIG64> cell;
    if (STAGED) {
        cell.mu = sh + c * pitch;
        cell.sg = sh + ((long long)p.tile + c) * pitch;
        cell.stride = 1;
    } else {
        const long long off = cell_off(p, c0 + c);
        cell.mu = static_cast<const V*>(p.mu) + off;
        cell.sg = SIG64 ? nullptr : static_cast<const V*>(p.sg) + off;
        cell.stride = p.col_stride;
    }
    cell.sg64 = SIG64 ? p.sg64 + (c0 + c) % p.sigma_cols : nullptr;
    cell.sg_stride = p.sigma_cols;
    return cell;
}

// kFlagNaN: a mu of the cell is not finite; kFlagBadSigma: a sigma is not positive and finite (wave-uniform)
template <class C>
__device__ inline int cell_flags(const C& cell, int S, int lane) {
    int f = 0;
    for (int s = lane; s < S; s += 64) {
        const double m = cell.m(s), sd = cell.sd(s);
        if (!isfinite(m)) f |= kFlagNaN;
        if (!(sd > 0.0) || !isfinite(sd)) f |= kFlagBadSigma;
    }
    return wave_or(f);
}

// The tail mass and the density of the mixture at x: tail = (1/S) sum 0.5 erfc(-u / sqrt 2) (1 - that with `upper`: 0.5 erfc(+u / sqrt 2)),
// dens = (1/S) sum phi(u) / sigma, u = (x - mu) / sigma - one pass over S.
template <class C>
__device__ inline void mix_eval(const C& cell, int S, int lane, double x, bool upper, double& tail, double& dens) {
    double a = 0.0, d = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double sd = cell.sd(s);
        const double u = (x - cell.m(s)) / sd;
        a += erfc((upper ? u : -u) * kInvSqrt2);
        d += exp(-0.5 * (u * u)) / sd;
    }
    tail = 0.5 * wave_sum(a) / (double)S;
    dens = wave_sum(d) * kInvSqrt2Pi / (double)S;
}

// E|N(m, sd^2)| = 2 sd phi(m / sd) + m erf(m / (sd sqrt 2)); both terms are >= 0
__device__ inline double abs_moment(double m, double sd) {
    const double z = m / sd;
    return 2.0 * sd * (exp(-0.5 * (z * z)) * kInvSqrt2Pi) + m * erf(z * kInvSqrt2);
}

// The quantile of probability prob (z its standard normal quantile) of the cell; every lane returns the same bits.
template <class C>
__device__ inline double cell_quantile(const C& cell, int S, int lane, double prob, double z) {
    const bool upper = prob > 0.5;
    const double target = upper ? 1.0 - prob : prob;
    double lo = INFINITY, hi = -INFINITY;
    for (int s = lane; s < S; s += 64) {
        const double v = cell.m(s) + cell.sd(s) * z;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    // h(x) = F(x) - prob, formed on the tail that keeps its precision: increasing in x, negative to the left of the root
    double tail, dens;
    auto h_at = [&](double x) {
        mix_eval(cell, S, lane, x, upper, tail, dens);
        return upper ? target - tail : tail - target;
    };
    double hl = h_at(lo);
    double hh = hi > lo ? h_at(hi) : hl;
    double w = fmax(hi - lo, fmax(fmax(fabs(lo), fabs(hi)) * DBL_EPSILON, DBL_MIN));
    for (int k = 0; k < kMixMaxWiden && hl > 0.0; ++k) {          // lo lies right of the root: it is an upper end
        hi = lo; hh = hl;
        lo -= w; w += w;
        hl = h_at(lo);
    }
    for (int k = 0; k < kMixMaxWiden && hh < 0.0; ++k) {          // hi lies left of the root: it is a lower end
        lo = hi; hl = hh;
        hi += w; w += w;
        hh = h_at(hi);
    }
    double x = NAN;                                                // (the first step bisects)
    for (int it = 0; it < kMixMaxSteps && hl != 0.0 && hh != 0.0; ++it) {
        if (!(x > lo && x < hi)) {
            x = lo + 0.5 * (hi - lo);
            if (!(x > lo && x < hi)) break;                        // the bracket cannot narrow
        }
        const double h = h_at(x);
        if (h < 0.0) { lo = x; hl = h; }
        else { hi = x; hh = h; }                                   // (h == 0: the loop ends, and hi is returned)
        x -= h / dens;                                             // (a density of 0 leaves the bracket: NaN or infinite)
    }
    // the end of the bracket with the smaller residual - not the smallest residual met on the way: where F is flat a point far from
    // the root has a small one
    return fabs(hl) <= fabs(hh) ? lo : hi;
}

template <class V, bool SIG64, bool STAGED>
__global__ __launch_bounds__(kStackThreads) void mixture_quantile_kernel(MixParams p) {
    extern __shared__ __align__(16) unsigned char mix_lds[];
    const V* sh = reinterpret_cast<const V*>(mix_lds);
    const int pitch = p.S | 1;
    const long long c0 = (long long)blockIdx.x * p.tile;
    const int tc = (int)min((long long)p.tile, p.n_cols - c0);
    if (STAGED) stage_tile<V, SIG64>(p, reinterpret_cast<V*>(mix_lds), c0, tc, pitch);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < tc; c += kStackWaves) {
        const Cell<V, SIG64> cell = cell_of<V, SIG64, STAGED>(p, sh, c0, c, pitch);
        const int f = cell_flags(cell, p.S, lane);
        if (f) {                                                   // (refused by the host: no search on such values)
            if (lane == 0) {
                atomicOr(p.flag, f);
                if (p.mean) p.mean[c0 + c] = NAN;
                for (int q = 0; q < p.n_probs; ++q) p.quantile[(long long)q * p.n_cols + c0 + c] = NAN;
            }
            continue;
        }
        if (p.mean) {
            const double K = cell.m(0);
            double s1 = 0.0;
            for (int s = lane; s < p.S; s += 64) s1 += cell.m(s) - K;
            s1 = wave_sum(s1);
            if (lane == 0) p.mean[c0 + c] = K + s1 / (double)p.S;
        }
        for (int q = 0; q < p.n_probs; ++q) {
            const double x = cell_quantile(cell, p.S, lane, p.p[q], p.z[q]);
            if (lane == 0) p.quantile[(long long)q * p.n_cols + c0 + c] = x;
        }
    }
}

template <class V, bool SIG64, bool STAGED>
__global__ __launch_bounds__(kStackThreads) void mixture_crps_kernel(MixParams p) {
    extern __shared__ __align__(16) unsigned char mix_lds[];
    const V* sh = reinterpret_cast<const V*>(mix_lds);
    const int pitch = p.S | 1;
    const long long c0 = (long long)blockIdx.x * p.tile;
    const int tc = (int)min((long long)p.tile, p.n_cols - c0);
    if (STAGED) stage_tile<V, SIG64>(p, reinterpret_cast<V*>(mix_lds), c0, tc, pitch);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = p.S;
    for (int c = wave; c < tc; c += kStackWaves) {
        const Cell<V, SIG64> cell = cell_of<V, SIG64, STAGED>(p, sh, c0, c, pitch);
        const int f = cell_flags(cell, S, lane);
        if (f) {
            if (lane == 0) {
                atomicOr(p.flag, f);
                p.crps[c0 + c] = NAN;
            }
            continue;
        }
        const double y = p.y[c0 + c];
        // the single term and the diagonal of the pair term: lanes stride over s
        double a1 = 0.0, dg = 0.0;
        for (int s = lane; s < S; s += 64) {
            const double sd = cell.sd(s);
            a1 += abs_moment(y - cell.m(s), sd);
            dg += kTwoOverSqrtPi * sd;
        }
        // the pairs s < t, row-major (row s holds t = s + 1 .. S - 1): lanes stride over the flat pair index
        double a2 = 0.0;
        int s = 0, i = lane;
        while (s < S - 1 && i >= S - 1 - s) { i -= S - 1 - s; ++s; }
        while (s < S - 1) {
            const int t = s + 1 + i;
            a2 += abs_moment(cell.m(s) - cell.m(t), hypot(cell.sd(s), cell.sd(t)));
            i += 64;
            while (s < S - 1 && i >= S - 1 - s) { i -= S - 1 - s; ++s; }
        }
        const double t1 = wave_sum(a1) / (double)S;
        const double t2 = (wave_sum(dg) + 2.0 * wave_sum(a2)) / ((double)S * (double)S);
        if (lane == 0) p.crps[c0 + c] = t1 - 0.5 * t2;
    }
}

// The sums of crps [n_rows][T] over the rows per target: the workgroup's partials part[T][gridDim.x], target by target.
__global__ __launch_bounds__(kFiThreads) void crps_totals_kernel(const double* __restrict__ crps, long long n_rows, int T, double* __restrict__ part) {
    __shared__ double red[kFiWaves];
    for (int t = 0; t < T; ++t) {
        double v = 0.0;
        for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) v += crps[r * T + t];
        const double a = block_sum(v, red);
        if (threadIdx.x == 0) part[(long long)t * gridDim.x + blockIdx.x] = a;
    }
}

// The standard normal quantile of prob: Newton on libm's erfc from 0 on the tail min(prob, 1 - prob) <= 0.5, where Phi is convex and
// the iterates fall monotonically onto the root.
double normal_quantile(double prob) {
    const bool upper = prob > 0.5;
    const double target = upper ? 1.0 - prob : prob;
    double z = 0.0;
    for (int it = 0; it < 200; ++it) {
        const double f = 0.5 * erfc(-z * kInvSqrt2) - target;
        const double step = f / (kInvSqrt2Pi * exp(-0.5 * z * z));
        if (!(fabs(step) > 1e-16 * fabs(z))) break;
        z -= step;
    }
    return upper ? -z : z;
}

// What both entries check of the probabilities and the outputs; fills p->p, p->z, p->n_probs.
int check_probs(npbnn_ctx* ctx, const char* who, const double* probs, int n_probs, const double* out_quantile, MixParams* p) {
    if (n_probs < 0 || n_probs > kMixMaxProbs) return fail(ctx, NPBNN_E_ARG, "%s: %d probabilities, at most %d", who, n_probs, kMixMaxProbs);
    if ((n_probs > 0) != (out_quantile != nullptr) || (n_probs > 0 && !probs))
        return fail(ctx, NPBNN_E_ARG, "%s: probs, n_probs and out_quantile go together (out_quantile is NULL with n_probs == 0)", who);
    for (int q = 0; q < kMixMaxProbs; ++q) p->p[q] = p->z[q] = 0.0;
    for (int q = 0; q < n_probs; ++q) {
        if (!(fmin(probs[q], 1.0 - probs[q]) >= kMinTail))
            return fail(ctx, NPBNN_E_ARG, "%s: probability %d is %g; min(p, 1 - p) must be at least %g", who, q, probs[q], kMinTail);
        p->p[q] = probs[q];
        p->z[q] = normal_quantile(probs[q]);
    }
    p->n_probs = n_probs;
    return NPBNN_OK;
}

// The kernels over the n_cols cells p describes (mu, sg / sg64, strides, S, probabilities, outputs; all on the device): the
// quantile kernel when quantiles or the mean are asked for, the CRPS kernel when p.crps is.  The caller reads the flag word.
template <class V, bool SIG64>
int launch_mixture(npbnn_ctx* ctx, hipStream_t stream, const MixParams& p) {
    const size_t cell_bytes = (size_t)(p.S | 1) * sizeof(V) * (SIG64 ? 1 : 2);
    int rc = NPBNN_OK;
    if (p.n_probs > 0 || p.mean)
        rc = launch_stack_kernel(ctx, stream, reinterpret_cast<const void*>(mixture_quantile_kernel<V, SIG64, true>),
                                 reinterpret_cast<const void*>(mixture_quantile_kernel<V, SIG64, false>), cell_bytes, p);
    if (!rc && p.crps)
        rc = launch_stack_kernel(ctx, stream, reinterpret_cast<const void*>(mixture_crps_kernel<V, SIG64, true>),
                                 reinterpret_cast<const void*>(mixture_crps_kernel<V, SIG64, false>), cell_bytes, p);
    return rc;
}
// f32: mu (and a same-type sigma) are float32
int launch_mixture(npbnn_ctx* ctx, hipStream_t stream, const MixParams& p, bool f32) {
    if (p.sigma_cols > 0) return f32 ? launch_mixture<float, true>(ctx, stream, p) : launch_mixture<double, true>(ctx, stream, p);
    return f32 ? launch_mixture<float, false>(ctx, stream, p) : launch_mixture<double, false>(ctx, stream, p);
}

int refuse_flags(npbnn_ctx* ctx, const char* who, int flags, const char* what) {
    if (flags & kFlagNaN) return fail(ctx, NPBNN_E_ARG, "%s: a %s is NaN or infinite", who, what);
    if (flags & kFlagBadSigma)
        return fail(ctx, NPBNN_E_ARG, "%s: a sigma is not positive and finite (a softplus that underflows to 0 in float32 is refused, not divided by)", who);
    return NPBNN_OK;
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_op_mixture(int device, const void* mu, const void* sigma, int value_type, int64_t n_samples, int64_t n_cols, int64_t col_stride,
                                int32_t sigma_cols, const double* probs, int32_t n_probs, const double* y, double* out_quantile, double* out_mean,
                                double* out_crps) {
    const char* who = "op_mixture";
    StackInput d_mu(value_type), d_sg(sigma_cols > 0 ? NPBNN_VALUE_F64 : value_type);
    if (!mu || !sigma || n_cols < 0 || col_stride < n_cols || n_samples < 1 || sigma_cols < 0 || !d_mu.ok())
        return fail(nullptr, NPBNN_E_ARG, "%s: bad arguments", who);
    if (n_samples > kStackMaxSamples) return fail(nullptr, NPBNN_E_ARG, "%s: %lld samples, at most %d", who, (long long)n_samples, kStackMaxSamples);
    MixParams p{};
    int rc = check_probs(nullptr, who, probs, n_probs, out_quantile, &p);
    if (rc) return rc;
    if ((y != nullptr) != (out_crps != nullptr)) return fail(nullptr, NPBNN_E_ARG, "%s: y and out_crps go together", who);
    if (!out_quantile && !out_mean && !out_crps) return fail(nullptr, NPBNN_E_ARG, "%s: nothing asked for", who);
    const bool f32 = d_mu.f32();
    auto value_at = [f32](const void* a, size_t i) { return f32 ? (double)static_cast<const float*>(a)[i] : static_cast<const double*>(a)[i]; };
    for (int64_t s = 0; s < n_samples; ++s)
        for (int64_t c = 0; c < n_cols; ++c) {
            const size_t at = (size_t)s * col_stride + c;
            if (!std::isfinite(value_at(mu, at))) return fail(nullptr, NPBNN_E_ARG, "%s: a mu is NaN or infinite", who);
            if (sigma_cols == 0 && (!(value_at(sigma, at) > 0.0) || !std::isfinite(value_at(sigma, at))))
                return fail(nullptr, NPBNN_E_ARG, "%s: a sigma is not positive and finite", who);
        }
    if (sigma_cols > 0 && (rc = check_sigma_sets(nullptr, who, static_cast<const double*>(sigma), (int)n_samples, sigma_cols))) return rc;
    for (int64_t c = 0; y && c < n_cols; ++c)
        if (!std::isfinite(y[c])) return fail(nullptr, NPBNN_E_ARG, "%s: a y is NaN or infinite", who);
    if (n_cols == 0) return NPBNN_OK;
    HIP_TRY(nullptr, hipSetDevice(device));
    DevBuf<double> d_y, d_out;
    DevBuf<int> d_flag;
    const size_t nq = (size_t)n_probs * n_cols;
    if ((rc = d_mu.upload(mu, n_samples, n_cols, col_stride))) return rc;
    if ((rc = sigma_cols > 0 ? d_sg.upload(sigma, n_samples, sigma_cols, sigma_cols) : d_sg.upload(sigma, n_samples, n_cols, col_stride))) return rc;
    if ((rc = dev_alloc(nullptr, d_y, y ? (size_t)n_cols : 0))) return rc;
    if ((rc = dev_alloc(nullptr, d_out, nq + 2 * (size_t)n_cols))) return rc;
    if ((rc = dev_alloc(nullptr, d_flag, 1))) return rc;
    if (y) HIP_TRY(nullptr, hipMemcpy(d_y.get(), y, (size_t)n_cols * 8, hipMemcpyHostToDevice));
    HIP_TRY(nullptr, hipMemset(d_flag.get(), 0, sizeof(int)));
    p.mu = d_mu.buf.get();
    p.sg = sigma_cols > 0 ? nullptr : d_sg.buf.get();
    p.sg64 = sigma_cols > 0 ? d_sg.buf.get() : nullptr;
    p.n_cols = n_cols;
    p.col_stride = col_stride;
    p.cells_per_row = 1;
    p.row_pitch = 1;
    p.S = (int)n_samples;
    p.sigma_cols = sigma_cols;
    p.y = d_y.get();
    p.quantile = out_quantile ? d_out.get() : nullptr;
    p.mean = out_mean ? d_out.get() + nq : nullptr;
    p.crps = out_crps ? d_out.get() + nq + n_cols : nullptr;
    p.flag = d_flag.get();
    if ((rc = launch_mixture(nullptr, nullptr, p, f32))) return rc;
    int flags = 0;
    HIP_TRY(nullptr, hipMemcpy(&flags, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost));
    if ((rc = refuse_flags(nullptr, who, flags, "mu"))) return rc;
    if (out_quantile) HIP_TRY(nullptr, hipMemcpy(out_quantile, p.quantile, nq * 8, hipMemcpyDeviceToHost));
    if (out_mean) HIP_TRY(nullptr, hipMemcpy(out_mean, p.mean, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    if (out_crps) HIP_TRY(nullptr, hipMemcpy(out_crps, p.crps, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
    return NPBNN_OK;
}

extern "C" int npbnn_predict_sets_predictive(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                             const double* sigma_sets, const double* probs, int32_t n_probs, const double* targets,
                                             double* out_quantile, double* out_mean, double* out_crps, double* out_totals) {
    const char* who = "predict_sets_predictive";
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || n_sets < 1) return fail(ctx, NPBNN_E_ARG, "%s: bad arguments", who);
    if (n_sets > kStackMaxSamples) return fail(ctx, NPBNN_E_ARG, "%s: %d samples, at most %d", who, n_sets, kStackMaxSamples);
    MixParams p{};
    int rc = check_probs(ctx, who, probs, n_probs, out_quantile, &p);
    if (rc) return rc;
    if (!targets && (out_crps || out_totals)) return fail(ctx, NPBNN_E_ARG, "%s: out_crps and out_totals need targets", who);
    if (targets && !out_crps && !out_totals) return fail(ctx, NPBNN_E_ARG, "%s: targets given and neither out_crps nor out_totals", who);
    if (!out_quantile && !out_mean && !targets) return fail(ctx, NPBNN_E_ARG, "%s: nothing asked for", who);
    SetsTable tb;
    if ((rc = open_sets_table(ctx, who, which, &tb))) return rc;
    const int C = ctx->net.n_out;
    const int kind = ctx->arch.out_kind;
    const bool sp = kind == NPBNN_OUT_SOFTPLUS_HALF;
    if (kind != NPBNN_OUT_IDENTITY && !sp)
        return fail(ctx, NPBNN_E_ARG, "%s: the predictive distribution is that of a regression: NPBNN_OUT_IDENTITY or NPBNN_OUT_SOFTPLUS_HALF", who);
    if (sp && C % 2 != 0) return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_SOFTPLUS_HALF splits the outputs into means and sigmas, and %d is odd", who, C);
    if (sp && sigma_sets) return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_SOFTPLUS_HALF predicts its sigma: sigma_sets must be NULL", who);
    if (!sp && !sigma_sets) return fail(ctx, NPBNN_E_ARG, "%s: NPBNN_OUT_IDENTITY needs sigma_sets [n_sets][n_targets]", who);
    const int T = sp ? C / 2 : C;
    if (!sp && (rc = check_sigma_sets(ctx, who, sigma_sets, n_sets, T))) return rc;
    const long long n_rows = tb.n_rows;
    const size_t n_cells = (size_t)n_rows * T;
    for (size_t i = 0; targets && i < n_cells; ++i)
        if (!std::isfinite(targets[i])) return fail(ctx, NPBNN_E_ARG, "%s: target %zu of row %zu is NaN or infinite", who, i % T, i / T);
    hipStream_t st = tb.st;
    const size_t per_set = (size_t)n_rows * C;
    const size_t nq = (size_t)n_probs * n_cells;
    const int n_wg = tb.n_wg;
    DevBuf<float> stack;
    DevBuf<double> d_sig, d_y, d_out, d_part;
    DevBuf<int> d_flag;
    // (with the output function applied a row of the stack holds T means followed by T sigmas; the identity has none to apply)
    if ((rc = replay_into_stack(ctx, who, W_sets, act_prm_sets, n_sets, which, sp ? 1 : 0, tb, &stack))) return rc;
    if ((rc = dev_alloc(ctx, d_sig, sp ? 0 : (size_t)n_sets * T))) return rc;
    if ((rc = dev_alloc(ctx, d_y, targets ? n_cells : 0))) return rc;
    if ((rc = dev_alloc(ctx, d_out, nq + 2 * n_cells))) return rc;
    if ((rc = dev_alloc(ctx, d_part, (size_t)T * n_wg))) return rc;
    if ((rc = dev_alloc(ctx, d_flag, 1))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_flag.get(), 0, sizeof(int), st));
    if (!sp) HIP_TRY(ctx, hipMemcpyAsync(d_sig.get(), sigma_sets, (size_t)n_sets * T * sizeof(double), hipMemcpyHostToDevice, st));
    if (targets) HIP_TRY(ctx, hipMemcpyAsync(d_y.get(), targets, n_cells * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                          // (sigma_sets and targets are pageable memory of the caller's)
    p.mu = stack.get();
    p.sg = sp ? stack.get() + T : nullptr;
    p.sg64 = sp ? nullptr : d_sig.get();
    p.n_cols = (long long)n_cells;
    p.col_stride = (long long)per_set;
    p.cells_per_row = T;
    p.row_pitch = C;
    p.S = n_sets;
    p.sigma_cols = sp ? 0 : T;
    p.y = d_y.get();
    p.quantile = out_quantile ? d_out.get() : nullptr;
    p.mean = out_mean ? d_out.get() + nq : nullptr;
    p.crps = targets ? d_out.get() + nq + n_cells : nullptr;
    p.flag = d_flag.get();
    if ((rc = launch_mixture(ctx, st, p, true))) return rc;
    if (out_totals) {
        hipLaunchKernelGGL(crps_totals_kernel, dim3((unsigned)n_wg), dim3(kFiThreads), 0, st, (const double*)p.crps, n_rows, T, d_part.get());
        HIP_TRY(ctx, hipGetLastError());
    }
    int flags = 0;
    std::vector<double> sums;
    if ((rc = fetch_flags_and_totals(ctx, d_flag.get(), d_part.get(), out_totals ? (size_t)T : 0, n_wg, &flags, &sums))) return rc;
    if ((rc = refuse_flags(ctx, who, flags, "prediction"))) return rc;
    if (out_totals) memcpy(out_totals, sums.data(), (size_t)T * sizeof(double));
    if (out_quantile) HIP_TRY(ctx, hipMemcpyAsync(out_quantile, p.quantile, nq * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_mean) HIP_TRY(ctx, hipMemcpyAsync(out_mean, p.mean, n_cells * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_crps) HIP_TRY(ctx, hipMemcpyAsync(out_crps, p.crps, n_cells * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
