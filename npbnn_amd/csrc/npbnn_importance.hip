// Permutation importance on the device (include/npbnn_hip.h): feature_importance of np_bnn/BNN_lib.py:504-597 asks, per permutation of a
// block of feature columns, for one accuracy - get_posterior_cat_prob's shuffle (:364-371), its loop over RunPredict (:375-381), its
// summary (:382-392) and CalcAccuracy (:203-209).
//
// npbnn_permute_columns: the shuffle is a row gather of a few columns.  The library keeps the moved columns as npbnn_set_data left them
// (Dataset::perm_saved, column-major [column][row]: save and gather read and write it coalesced); a call puts the previous call's columns
// back, saves the new ones and gathers from the SAVED copy into X, so no workgroup reads what another one writes.  The fp16-split copies
// (X16 row-major, X16w in the weight-streamed path's piece order) are patched in the 8-feature groups that hold a moved column, with the
// arithmetic of split_x_kernel / split_x_tiled_kernel under the scales the copies were built with: bit for bit what a fresh split of the
// permuted matrix writes, since a column's largest entry - all its scale depends on - does not move with its rows.  Row indices are
// checked by a kernel of their own before anything is written.
//
// npbnn_predict_sets_summary: the sets replay as in npbnn_predict_sets (groups that share their slopes, the float32 retry; the replay
// is replay_sets_accumulate, which npbnn_predict_sets_support of npbnn_support.hip and, in a mode of its own, npbnn_predict_sets_lppd of
// npbnn_lppd.hip call too); after each
// group summary_accumulate_kernel folds the group's float32 predictions [g][rows][C] into uint32 votes (mode 0: per set and row the
// first class holding the row's maximum - numpy's argmax) or float64 sums (mode 1: set after set - the order np.mean(axis=0) adds a
// C-contiguous [S, N, C] array in).  Streaming: g x N x C floats in, N x C accumulators in and out, one thread per row (mode 0) or per
// four (row, class) entries (mode 1), 16-byte accesses where C allows.  summary_final_kernel divides by the number of sets, takes each
// row's first argmax of the QUOTIENT (a division can turn an inequality into a tie) and counts [label][argmax] in an LDS histogram
// with integer atomics, one global integer atomic per nonzero cell and workgroup: the table does not depend on the order.
#include "npbnn_sets.hip.h"

#include <vector>

namespace npbnn_api {

namespace {

constexpr int kConfLdsClasses = 64;                // confusion tables up to this many classes are counted in LDS first (16 KiB)

// ---- permutation -------------------------------------------------------------------------------

__global__ __launch_bounds__(kFiThreads) void perm_check_kernel(const long long* __restrict__ perm, long long n, long long n_rows, int* __restrict__ flag) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFiThreads) {
        const long long v = perm[i];
        if (v < 0 || v >= n_rows) bad = true;
    }
    if (bad) atomicOr(flag, kFlagBadRow);
}

// X[r][cols[j]] = saved[j][r]: the columns a previous call moved go back
__global__ __launch_bounds__(kFiThreads) void perm_restore_kernel(float* __restrict__ X, int Fp, long long n_rows, const int* __restrict__ cols, int n_cols,
                                                                  const float* __restrict__ saved) {
    const long long n = n_rows * n_cols;
    for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFiThreads) {
        const int j = (int)(i / n_rows);
        const long long r = i - (long long)j * n_rows;
        X[r * Fp + cols[j]] = saved[i];
    }
}

// saved[j][r] = X[r][cols[j]]
__global__ __launch_bounds__(kFiThreads) void perm_save_kernel(const float* __restrict__ X, int Fp, long long n_rows, const int* __restrict__ cols, int n_cols,
                                                               float* __restrict__ saved) {
    const long long n = n_rows * n_cols;
    for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFiThreads) {
        const int j = (int)(i / n_rows);
        const long long r = i - (long long)j * n_rows;
        saved[i] = X[r * Fp + cols[j]];
    }
}

// X[r][cols[j]] = saved[j][perm[p][r]], p = 0 (one permutation for the block) or j.  Reads the saved copy only (indices checked by
// perm_check_kernel), writes X only.
__global__ __launch_bounds__(kFiThreads) void perm_gather_kernel(float* __restrict__ X, int Fp, long long n_rows, const int* __restrict__ cols, int n_cols,
                                                                 const float* __restrict__ saved, const long long* __restrict__ perm, int per_column) {
    const long long n = n_rows * n_cols;
    for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFiThreads) {
        const int j = (int)(i / n_rows);
        const long long r = i - (long long)j * n_rows;
        const long long src = perm[(per_column ? (long long)j * n_rows : 0) + r];
        X[r * Fp + cols[j]] = saved[(long long)j * n_rows + src];
    }
}

// The 8-feature groups `groups` of the fp16-split copies, split again from X for the rows below n_rows (the padding rows stay zero):
// split_x_kernel's arithmetic into X16 (when given) and split_x_tiled_kernel's placement into X16w (when given).
__global__ __launch_bounds__(kFiThreads) void perm_patch_split_kernel(const float* __restrict__ X, long long n_rows, int Fp, const int* __restrict__ groups,
                                                                      int n_groups, const float* __restrict__ x_scale, float* __restrict__ X16, int Fp16,
                                                                      float* __restrict__ X16w, int n_units) {
    const long long n = n_rows * n_groups;
    for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFiThreads) {
        const long long r = i / n_groups;
        const int grp = groups[(int)(i - r * n_groups)], c0 = grp * 8;
        f16x8 hi, lo;
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            const float v = c < Fp ? X[r * Fp + c] * x_scale[c] : 0.f;
            _Float16 h, l;
            split_f16(v, h, l);
            hi[j] = h;
            lo[j] = l;
        }
        if (X16 && c0 < Fp16) {
            f16x8* dst = reinterpret_cast<f16x8*>(X16 + r * Fp16 + c0);
            dst[0] = hi;
            dst[1] = lo;
        }
        if (X16w && grp < n_units * 4) {
            const long long T = r >> 4;
            const int row = (int)(r & 15), u = grp >> 2, kg = grp & 3;
            float* piece = X16w + (((T * n_units + u) * 2) + (kg >> 1)) * 256;
            *reinterpret_cast<f16x8*>(piece + ((2 * (kg & 1)) * 16 + row) * 4) = hi;
            *reinterpret_cast<f16x8*>(piece + ((2 * (kg & 1) + 1) * 16 + row) * 4) = lo;
        }
    }
}

// ---- summary -----------------------------------------------------------------------------------

// mode 0: votes[r][k] += 1 for the first class k holding the maximum of set j's row r; one thread per row.  VEC: C is a multiple of
// 4, rows are read as float4.
template <bool VEC>
__global__ __launch_bounds__(kFiThreads) void summary_votes_kernel(const float* __restrict__ y, int g, long long n_rows, int C, unsigned* __restrict__ votes,
                                                                   int* __restrict__ flag) {
    bool nan = false;
    const long long per_set = n_rows * C;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        for (int j = 0; j < g; ++j) {
            const float* row = y + (long long)j * per_set + r * C;
            float best = 0.f;
            int bk = -1;
            if (VEC) {
                for (int k = 0; k < C; k += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        nan = nan || (v[q] != v[q]);
                        if (bk < 0 || v[q] > best) { best = v[q]; bk = k + q; }
                    }
                }
            } else {
                for (int k = 0; k < C; ++k) {
                    const float v = row[k];
                    nan = nan || (v != v);
                    if (bk < 0 || v > best) { best = v; bk = k; }
                }
            }
            votes[r * C + bk] += 1u;
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// mode 1: sum[i] += y[j][i] for j = 0 .. g - 1 in that order, float32 widened to float64.  VEC: rows x C is a multiple of 4, a thread
// owns four consecutive entries (one 16-byte read per set, two 16-byte reads and writes of the sums).
template <bool VEC>
__global__ __launch_bounds__(kFiThreads) void summary_sums_kernel(const float* __restrict__ y, int g, long long per_set, double* __restrict__ sum,
                                                                  int* __restrict__ flag) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    bool nan = false;
    if (VEC) {
        const long long n4 = per_set >> 2;
        for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kFiThreads) {
            f64x2* dst = reinterpret_cast<f64x2*>(sum + 4 * i);
            f64x2 a = dst[0], b = dst[1];
            for (int j = 0; j < g; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(y + (long long)j * per_set + 4 * i);
                nan = nan || (v[0] != v[0]) || (v[1] != v[1]) || (v[2] != v[2]) || (v[3] != v[3]);
                a[0] += (double)v[0];
                a[1] += (double)v[1];
                b[0] += (double)v[2];
                b[1] += (double)v[3];
            }
            dst[0] = a;
            dst[1] = b;
        }
    } else {
        for (long long i = (long long)blockIdx.x * kFiThreads + threadIdx.x; i < per_set; i += (long long)gridDim.x * kFiThreads) {
            double a = sum[i];
            for (int j = 0; j < g; ++j) {
                const float v = y[(long long)j * per_set + i];
                nan = nan || (v != v);
                a += (double)v;
            }
            sum[i] = a;
        }
    }
    if (nan) atomicOr(flag, kFlagNaN);
}

// One thread per row: the quotient accumulator / n_sets (ACC = unsigned votes or double sums) into `summary` (when given), the first
// class holding the row's largest quotient, and (labels given) confusion[label][that class] += 1 - through an LDS histogram when
// the table fits one (lds_conf), straight into the global table otherwise.
template <class ACC>
__global__ __launch_bounds__(kFiThreads) void summary_final_kernel(const ACC* __restrict__ acc, long long n_rows, int C, double n_sets,
                                                                   double* __restrict__ summary, const long long* __restrict__ labels,
                                                                   unsigned long long* __restrict__ confusion, int lds_conf, int* __restrict__ flag) {
    __shared__ unsigned hist[kConfLdsClasses * kConfLdsClasses];
    const int cells = C * C;
    if (labels && lds_conf) {
        for (int i = threadIdx.x; i < cells; i += kFiThreads) hist[i] = 0u;
        __syncthreads();
    }
    bool bad = false;
    for (long long r = (long long)blockIdx.x * kFiThreads + threadIdx.x; r < n_rows; r += (long long)gridDim.x * kFiThreads) {
        double best = 0.0;
        int bk = -1;
        for (int k = 0; k < C; ++k) {
            const double q = (double)acc[r * C + k] / n_sets;
            if (summary) summary[r * C + k] = q;
            if (bk < 0 || q > best) { best = q; bk = k; }
        }
        if (labels) {
            const long long lab = labels[r];
            if (lab < 0 || lab >= C) bad = true;
            else if (lds_conf) atomicAdd(&hist[(int)lab * C + bk], 1u);
            else atomicAdd(&confusion[lab * C + bk], 1ull);
        }
    }
    if (bad) atomicOr(flag, kFlagBadLabel);
    if (labels && lds_conf) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += kFiThreads) {
            const unsigned n = hist[i];
            if (n) atomicAdd(&confusion[i], (unsigned long long)n);
        }
    }
}

}  // namespace

}  // namespace npbnn_api

using namespace npbnn_api;

extern "C" int npbnn_permute_columns(npbnn_ctx* ctx, int which, const int32_t* cols, int32_t n_cols, const int64_t* perm, int32_t n_perm) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "permute_columns: which must be 0 or 1");
    Dataset& d = ctx->ds[which];
    if (!d.m->X) return fail(ctx, NPBNN_E_STATE, "permute_columns: call npbnn_set_data first");
    if (ctx->store_taken) return fail(ctx, NPBNN_E_STATE, "permute_columns: this context's matrices belong to another one (npbnn_share_data)");
    if (ctx->store.use_count() > 1)
        return fail(ctx, NPBNN_E_STATE, "permute_columns: %d other context(s) use this one's matrices (npbnn_share_data)", (int)ctx->store.use_count() - 1);
    if (n_cols < 0 || (n_cols > 0 && !cols)) return fail(ctx, NPBNN_E_ARG, "permute_columns: bad arguments");
    if (!perm) n_cols = 0;                   // (restore only)
    if (n_cols > 0 && n_perm != 1 && n_perm != n_cols)
        return fail(ctx, NPBNN_E_ARG, "permute_columns: %d permutations for %d columns (one for the block, or one per column)", n_perm, n_cols);
    std::vector<int> now(cols, cols + n_cols);
    {
        std::vector<char> seen((size_t)d.m->F, 0);
        for (int c : now) {
            if (c < 0 || c >= d.m->F) return fail(ctx, NPBNN_E_ARG, "permute_columns: column %d outside the matrix (%d features)", c, d.m->F);
            if (seen[(size_t)c]) return fail(ctx, NPBNN_E_ARG, "permute_columns: column %d named twice", c);
            seen[(size_t)c] = 1;
        }
    }
    if (now.empty() && d.perm_cols.empty()) return NPBNN_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long long n_rows = d.m->n_rows;
    const size_t n_old = d.perm_cols.size(), n_new = now.size();
    // the 8-feature groups of the split copies that a restored or a moved column lies in
    std::vector<int> groups;
    {
        std::vector<char> seen((size_t)(d.m->Fp / 8 + 4), 0);
        for (const std::vector<int>* v : {&d.perm_cols, &now})
            for (int c : *v)
                if (!seen[(size_t)(c / 8)]) { seen[(size_t)(c / 8)] = 1; groups.push_back(c / 8); }
    }
    // one upload: [old columns | new columns | groups], and the permutations
    std::vector<int> h_idx;
    h_idx.insert(h_idx.end(), d.perm_cols.begin(), d.perm_cols.end());
    h_idx.insert(h_idx.end(), now.begin(), now.end());
    h_idx.insert(h_idx.end(), groups.begin(), groups.end());
    DevBuf<int> d_idx, d_flag;
    DevBuf<long long> d_perm;
    int rc;
    if ((rc = d_idx.reserve(ctx, h_idx.size()))) return rc;
    if ((rc = d_flag.reserve(ctx, 4))) return rc;
    FiTimer tm;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, h_idx.data(), h_idx.size() * sizeof(int), hipMemcpyHostToDevice, st));
    const int* d_old = d_idx.get();
    const int* d_new = d_old + n_old;
    const int* d_groups = d_new + n_new;
    if (n_new) {
        const long long n_idx = (long long)n_perm * n_rows;
        if ((rc = d_perm.reserve(ctx, (size_t)n_idx))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_perm, perm, (size_t)n_idx * sizeof(long long), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
        hipLaunchKernelGGL(perm_check_kernel, dim3(grid_for(n_idx)), dim3(kFiThreads), 0, st, (const long long*)d_perm.get(), n_idx, n_rows, d_flag.get());
        HIP_TRY(ctx, hipGetLastError());
        int bad = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&bad, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (bad) return fail(ctx, NPBNN_E_ARG, "permute_columns: a row index lies outside [0, %lld)", n_rows);
    }
    tm.mark(0, st);
    if (n_old) {
        hipLaunchKernelGGL(perm_restore_kernel, dim3(grid_for(n_rows * (long long)n_old)), dim3(kFiThreads), 0, st, d.m->X, d.m->Fp, n_rows, d_old, (int)n_old,
                           (const float*)d.perm_saved.get());
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_new) {
        // (the restore above has read the saved copy before this, in stream order, may replace it)
        DevBuf<float> fresh;
        if (d.perm_saved.size() < (size_t)n_rows * n_new) {
            if ((rc = fresh.reserve(ctx, (size_t)n_rows * n_new))) return rc;
        }
        float* saved = fresh ? fresh.get() : d.perm_saved.get();
        hipLaunchKernelGGL(perm_save_kernel, dim3(grid_for(n_rows * (long long)n_new)), dim3(kFiThreads), 0, st, (const float*)d.m->X, d.m->Fp, n_rows, d_new, (int)n_new,
                           saved);
        hipLaunchKernelGGL(perm_gather_kernel, dim3(grid_for(n_rows * (long long)n_new)), dim3(kFiThreads), 0, st, d.m->X, d.m->Fp, n_rows, d_new, (int)n_new,
                           (const float*)saved, (const long long*)d_perm.get(), n_perm == 1 ? 0 : 1);
        HIP_TRY(ctx, hipGetLastError());
        if (fresh) {
            HIP_TRY(ctx, hipStreamSynchronize(st));          // (the old copy is freed by the move: the restore must be through)
            d.perm_saved = std::move(fresh);
        }
    }
    float* x16 = (d.m->f16_state > 0) ? d.m->X16 : nullptr;
    if ((x16 || d.m->X16w) && ctx->store->xscale) {
        hipLaunchKernelGGL(perm_patch_split_kernel, dim3(grid_for(n_rows * (long long)groups.size())), dim3(kFiThreads), 0, st, (const float*)d.m->X, n_rows, d.m->Fp,
                           d_groups, (int)groups.size(), (const float*)ctx->store->xscale, x16, d.m->Fp16, d.m->X16w, (d.m->F + 31) / 32);
        HIP_TRY(ctx, hipGetLastError());
    }
    tm.mark(1, st);
    HIP_TRY(ctx, hipStreamSynchronize(st));                  // (d_idx / d_perm go out of scope)
    d.perm_cols = now;
    ctx->fi_ns[0] = tm.ns(0, 1);
    return NPBNN_OK;
}

int npbnn_api::replay_sets_accumulate(npbnn_ctx* ctx, const char* who, const double* W_sets, const double* act_prm_sets, int n_sets, int which,
                                      int apply_out_fn, int mode, double* d_acc, int* d_flag, const ReplayLppd* lppd, const ReplayUncertainty* unc) {
    if (mode == kReplayLppd && (!lppd || apply_out_fn)) return fail(ctx, NPBNN_E_INTERNAL, "%s: the log-likelihood replay takes pre-output values", who);
    if (mode == kReplayUncertainty && (!unc || apply_out_fn)) return fail(ctx, NPBNN_E_INTERNAL, "%s: the uncertainty replay takes pre-output values", who);
    Dataset& d = ctx->ds[which];
    const int C = ctx->net.n_out;
    const int n_act = ctx->net.n_layers - 1;
    const long long n_rows = d.m->n_rows;
    const size_t per_set = (size_t)n_rows * C;
    const size_t wn = (size_t)ctx->n_weights;
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = ctx->d_y.reserve(ctx, kMaxCand * per_set))) return rc;
    FiTimer tm;
    double pass_ns = 0.0, acc_ns = 0.0;
    std::vector<double> wstage(kMaxCand * wn);
    int s0 = 0;
    while (s0 < n_sets) {
        // sets that share their activation slopes travel together, up to kMaxCand per streaming read of X (npbnn_predict_sets)
        int g = 1;
        while (s0 + g < n_sets && g < kMaxCand &&
               (!act_prm_sets || n_act == 0 ||
                memcmp(act_prm_sets + (size_t)(s0 + g) * n_act, act_prm_sets + (size_t)s0 * n_act, (size_t)n_act * sizeof(double)) == 0))
            ++g;
        for (int attempt = 0; attempt < 2; ++attempt) {
            LaunchPlan lp;
            rc = plan_launch(ctx, which, &lp, attempt, g, true);
            if (rc) return rc;
            if (lp.n_cand < g) g = lp.n_cand;
            memcpy(wstage.data(), W_sets + (size_t)s0 * wn, (size_t)g * wn * sizeof(double));
            tm.mark(0, st);
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_wraw, wstage.data(), (size_t)g * wn * sizeof(double), hipMemcpyHostToDevice, st));
            for (int l = 0; l < kMaxLayers; ++l) ctx->net.act_prm[l] = 0.f;
            if (act_prm_sets)
                for (int l = 0; l < n_act; ++l) ctx->net.act_prm[l] = (float)act_prm_sets[(size_t)s0 * n_act + l];
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_overflow, 0, sizeof(int), st));
            for (int j = 0; j < g; ++j)
                launch_pack_weights(ctx, ctx->d_wraw + (size_t)j * wn, nullptr, ctx->d_image + (size_t)j * ctx->net.image_floats, ctx->d_overflow);
            HIP_TRY(ctx, hipGetLastError());
            EvalParams p = make_params(ctx, d);
            p.labels = nullptr;
            p.targets = nullptr;
            p.net.lik_kind = NPBNN_LIK_NONE;
            p.y_out = ctx->d_y;
            p.predict_mode = apply_out_fn ? 2 : 1;
            p.weight_sets = 1;
            p.lay = layout_for(ctx, d, true);
            rc = push_eval_params(ctx, p);
            if (rc) return rc;
            rc = launch_plain_eval(ctx, lp, which);
            if (rc) return rc;
            HIP_TRY(ctx, hipGetLastError());
            tm.mark(1, st);
            int ovf = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&ovf, ctx->d_overflow, sizeof(int), hipMemcpyDeviceToHost, st));
            // (push_eval_params stages through one pinned slot: the launch that reads it must be in before the next write)
            HIP_TRY(ctx, hipStreamSynchronize(st));
            pass_ns += tm.ns(0, 1);
            if (ovf & kFlagStructure) return fail(ctx, NPBNN_E_ARG, "%s: a layer-0 weight is not zero where the mask given to npbnn_set_layer_mask is", who);
            if (!(ctx->net.l0_f16 && (ovf & kFlagF16Range))) break;
            if (ctx->l0_option == NPBNN_L0_F16) return fail(ctx, NPBNN_E_RANGE, "%s: a layer-0 weight left the fp16 range", who);
        }
        // the group's predictions [g][rows][C] into the accumulator, before the next group overwrites them
        tm.mark(2, st);
        if (mode == kReplayLppd) {
            launch_lppd_accumulate(st, ctx->d_y.get(), g, s0, n_rows, C, d_acc, *lppd, d_flag);
        } else if (mode == kReplayUncertainty) {
            launch_uncertainty_accumulate(st, ctx->d_y.get(), g, s0, n_rows, C, d_acc, *unc, d_flag);
        } else if (mode == kReplayVotes) {
            unsigned* votes = reinterpret_cast<unsigned*>(d_acc);
            if (C % 4 == 0)
                hipLaunchKernelGGL(summary_votes_kernel<true>, dim3(grid_for(n_rows)), dim3(kFiThreads), 0, st, (const float*)ctx->d_y.get(), g, n_rows, C, votes, d_flag);
            else
                hipLaunchKernelGGL(summary_votes_kernel<false>, dim3(grid_for(n_rows)), dim3(kFiThreads), 0, st, (const float*)ctx->d_y.get(), g, n_rows, C, votes, d_flag);
        } else {
            if (per_set % 4 == 0)
                hipLaunchKernelGGL(summary_sums_kernel<true>, dim3(grid_for((long long)(per_set / 4))), dim3(kFiThreads), 0, st, (const float*)ctx->d_y.get(), g,
                                   (long long)per_set, d_acc, d_flag);
            else
                hipLaunchKernelGGL(summary_sums_kernel<false>, dim3(grid_for((long long)per_set)), dim3(kFiThreads), 0, st, (const float*)ctx->d_y.get(), g,
                                   (long long)per_set, d_acc, d_flag);
        }
        HIP_TRY(ctx, hipGetLastError());
        tm.mark(3, st);
        if (tm.on) {
            HIP_TRY(ctx, hipStreamSynchronize(st));
            acc_ns += tm.ns(2, 3);
        }
        s0 += g;
    }
    ctx->fi_ns[1] = pass_ns > (double)INT_MAX ? INT_MAX : (int)pass_ns;
    ctx->fi_ns[2] = acc_ns > (double)INT_MAX ? INT_MAX : (int)acc_ns;
    return NPBNN_OK;
}

extern "C" int npbnn_predict_sets_summary(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                          int apply_out_fn, int mode, const int64_t* labels, double* out_summary, int64_t* out_confusion) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || n_sets < 1 || (!out_summary && !out_confusion) || (out_confusion != nullptr) != (labels != nullptr))
        return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: bad arguments");
    if (mode != 0 && mode != 1) return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: mode must be 0 (votes) or 1 (mean), got %d", mode);
    if (which != 0 && which != 1) return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: which must be 0 or 1");
    if (!ctx->arch_set) return fail(ctx, NPBNN_E_STATE, "predict_sets_summary: call npbnn_set_arch first");
    Dataset& d = ctx->ds[which];
    int rc = check_dataset_for_lik(ctx, d, NPBNN_LIK_NONE);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int C = ctx->net.n_out;
    const long long n_rows = d.m->n_rows;
    const size_t per_set = (size_t)n_rows * C;
    hipStream_t st = ctx->stream;
    // accumulators (per_set doubles, or as many unsigned), the summary, the confusion table, the labels, the flag word
    DevBuf<double> d_acc, d_summary;
    DevBuf<unsigned long long> d_conf;
    DevBuf<long long> d_labels;
    DevBuf<int> d_flag;
    if ((rc = d_acc.reserve(ctx, per_set))) return rc;
    if ((rc = d_flag.reserve(ctx, 4))) return rc;
    if (out_summary && (rc = d_summary.reserve(ctx, per_set))) return rc;
    if (labels) {
        if ((rc = d_conf.reserve(ctx, (size_t)C * C))) return rc;
        if ((rc = d_labels.reserve(ctx, (size_t)n_rows))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_labels, labels, (size_t)n_rows * sizeof(long long), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(d_conf, 0, (size_t)C * C * sizeof(unsigned long long), st));
    }
    HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, per_set * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    rc = replay_sets_accumulate(ctx, "predict_sets_summary", W_sets, act_prm_sets, n_sets, which, apply_out_fn, mode, d_acc.get(), d_flag.get());
    if (rc) return rc;
    FiTimer tm;
    tm.mark(0, st);
    const int lds_conf = C <= kConfLdsClasses ? 1 : 0;
    const long long* lab = labels ? d_labels.get() : nullptr;
    double* summary = out_summary ? d_summary.get() : nullptr;
    if (mode == 0)
        hipLaunchKernelGGL(summary_final_kernel<unsigned>, dim3(grid_for(n_rows)), dim3(kFiThreads), 0, st, (const unsigned*)reinterpret_cast<unsigned*>(d_acc.get()),
                           n_rows, C, (double)n_sets, summary, lab, d_conf.get(), lds_conf, d_flag.get());
    else
        hipLaunchKernelGGL(summary_final_kernel<double>, dim3(grid_for(n_rows)), dim3(kFiThreads), 0, st, (const double*)d_acc.get(), n_rows, C, (double)n_sets,
                           summary, lab, d_conf.get(), lds_conf, d_flag.get());
    HIP_TRY(ctx, hipGetLastError());
    tm.mark(1, st);
    int flags = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flags, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->fi_ns[3] = tm.ns(0, 1);
    if (flags & kFlagNaN) return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: a prediction is NaN");
    if (flags & kFlagBadLabel) return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: a label lies outside [0, %d)", C);
    if (out_summary) HIP_TRY(ctx, hipMemcpyAsync(out_summary, summary, per_set * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_confusion) HIP_TRY(ctx, hipMemcpyAsync(out_confusion, d_conf, (size_t)C * C * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
