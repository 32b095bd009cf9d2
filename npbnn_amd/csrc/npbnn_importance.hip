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
// npbnn_predict_sets_summary: the sets replay through replay_sets (npbnn_sets.hip.h: groups that share their slopes, the float32
// retry); after each group launch_summary_accumulate, which npbnn_predict_sets_support of npbnn_support.hip calls too, folds the
// group's float32 predictions [g][rows][C] into uint32 votes (mode 0: per set and row the first class holding the row's maximum -
// numpy's argmax) or float64 sums (mode 1: set after set - the order np.mean(axis=0) adds a C-contiguous [S, N, C] array in).
// Streaming: g x N x C floats in, N x C accumulators in and out, one thread per row (mode 0) or per four (row, class) entries (mode 1),
// 16-byte accesses where C allows.  summary_final_kernel divides by the number of sets, takes each row's first argmax of the QUOTIENT
// (a division can turn an inequality into a tie) and counts [label][argmax] in an LDS histogram with integer atomics, one global
// integer atomic per nonzero cell and workgroup: the table does not depend on the order.
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

void launch_summary_accumulate(hipStream_t st, const float* y, int g, long long n_rows, int C, int mode, double* d_acc, int* d_flag) {
    const dim3 block(kFiThreads);
    const long long per_set = n_rows * C;
    if (mode == 0) {
        unsigned* votes = reinterpret_cast<unsigned*>(d_acc);
        if (C % 4 == 0) hipLaunchKernelGGL(summary_votes_kernel<true>, dim3(grid_for(n_rows)), block, 0, st, y, g, n_rows, C, votes, d_flag);
        else hipLaunchKernelGGL(summary_votes_kernel<false>, dim3(grid_for(n_rows)), block, 0, st, y, g, n_rows, C, votes, d_flag);
    } else {
        if (per_set % 4 == 0) hipLaunchKernelGGL(summary_sums_kernel<true>, dim3(grid_for(per_set / 4)), block, 0, st, y, g, per_set, d_acc, d_flag);
        else hipLaunchKernelGGL(summary_sums_kernel<false>, dim3(grid_for(per_set)), block, 0, st, y, g, per_set, d_acc, d_flag);
    }
}

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

extern "C" int npbnn_predict_sets_summary(npbnn_ctx* ctx, const double* W_sets, const double* act_prm_sets, int32_t n_sets, int which,
                                          int apply_out_fn, int mode, const int64_t* labels, double* out_summary, int64_t* out_confusion) {
    if (!ctx) return fail(nullptr, NPBNN_E_ARG, "null ctx");
    if (!W_sets || n_sets < 1 || (!out_summary && !out_confusion) || (out_confusion != nullptr) != (labels != nullptr))
        return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: bad arguments");
    if (mode != 0 && mode != 1) return fail(ctx, NPBNN_E_ARG, "predict_sets_summary: mode must be 0 (votes) or 1 (mean), got %d", mode);
    SetsTable tb;
    int rc = open_sets_table(ctx, "predict_sets_summary", which, &tb);
    if (rc) return rc;
    const int C = ctx->net.n_out;
    const long long n_rows = tb.n_rows;
    const size_t per_set = (size_t)n_rows * C;
    hipStream_t st = tb.st;
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
    rc = replay_sets(ctx, "predict_sets_summary", W_sets, act_prm_sets, n_sets, which, apply_out_fn, nullptr, [&](const SetGroup& grp) {
        launch_summary_accumulate(st, grp.y, grp.g, n_rows, C, mode, d_acc.get(), d_flag.get());
        return NPBNN_OK;
    });
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
    std::vector<double> none;                      // (no floating-point partials: the tables are integers)
    if ((rc = finish_sets_entry(ctx, "predict_sets_summary", tm, d_flag.get(), nullptr, 0, 0, &ctx->fi_ns[3], C, &none))) return rc;
    if (out_summary) HIP_TRY(ctx, hipMemcpyAsync(out_summary, summary, per_set * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_confusion) HIP_TRY(ctx, hipMemcpyAsync(out_confusion, d_conf, (size_t)C * C * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return NPBNN_OK;
}
