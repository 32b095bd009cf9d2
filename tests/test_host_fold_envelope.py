"""The guards of tests/test_hip_fold_envelope.py, on the CPU: a plain numpy model of each set-statistic fold as the kernels lay it out
(npbnn_lppd.hip, npbnn_uncertainty.hip, npbnn_calibration.hip, npbnn_fold.hip.h) - accumulators [C][n_rows], the sets taken group
after group in run order, a group's accumulators reloaded when it is not the first, rows cut into workgroups of 256, one partial per
quantity and workgroup at part[q * n_wg + w], added in workgroup order - and the same model with one deliberate mistake.

The right model agrees with the float64 restatements of fold_envelope_cases on every case to HOST_TOL; every wrong one lies at least
WRONG_FACTOR bounds of the GPU test away from them on every case it applies to, and for every mistake the table has such a case.  So a
device fold with one of these mistakes cannot pass test_hip_fold_envelope.py, and an edit of the table cannot silently lose the case
that catches it.  The values folded are the float64 oracle's pre-output values rounded to float32.

The mistakes (``applies`` says where each can differ from the right fold at all):
  second_vector_reads_first   a float4 read at k >= 4 returns the vector at k - 4: the float4 builds with 8 or more outputs;
  class_index_drops_k         the softmax fold's class accumulator is indexed q, not k + q: its float4 build with 8 or more classes;
  second_pair_sigma           cal_regress_accumulate_kernel<SP, VEC> reads the second and later pairs' sigmas at T + t - 2: T >= 4;
  last_partial_dropped        the last workgroup's partials are not added: two or more workgroups;
  partial_stride_1            quantity q's partials are read at q + w, not q * n_wg + w: two or more workgroups;
  no_reload                   a group after the first starts from zeroed accumulators: two or more passes;
  group_first_is_K            every group's first set is taken as the row's first (j == 0 for s0 + j == 0): two or more passes, a fold
                              that keeps K (lppd, and the regression folds of the other two);
  train_labels                the training slot's labels or targets are read on the test table: lppd and calibration;
  train_row_count             the training slot's row count is used on the test table: 300 of the 513 rows are folded."""
import math

import numpy as np
import pytest

import fold_envelope_cases as fc
import uncertainty_cases as uc

VARIANTS = ("second_vector_reads_first", "class_index_drops_k", "second_pair_sigma", "last_partial_dropped", "partial_stride_1", "no_reload",
            "group_first_is_K", "train_labels", "train_row_count")
PAIRS = [(e, n) for e in fc.ENTRIES for n in fc.cases_of(e)]
# mistakes an entry's code cannot make: lppd keeps no class accumulators, only calibration reads pairs, uncertainty reads no labels
NOT_THIS_ENTRYS = {("class_index_drops_k", "lppd"), ("second_pair_sigma", "lppd"), ("second_pair_sigma", "uncertainty"), ("train_labels", "uncertainty")}


def applies(variant, entry, case):
    kind, n_out, vec = case["kind"], case["n_out"], case["n_out"] % 4 == 0
    passes = len(fc.inputs(case["name"])["groups"])
    if kind == "cat" and n_out == 1 and (entry == "lppd" or (entry == "uncertainty" and variant != "no_reload")):
        # the degenerate softmax: every log-likelihood and every entropy is 0 whatever is folded, dropped or misplaced; only the mean
        # probability, 1, shows a sum that starts over.  (Calibration's confidences of 1 show in its sums.)
        return False
    if variant == "second_vector_reads_first":      # (the pairs of calibration's means-plus-sigmas build are second_pair_sigma's)
        return vec and n_out >= 8 and not (entry == "calibration" and kind == "err")
    if variant == "class_index_drops_k":
        return kind == "cat" and entry != "lppd" and vec and n_out >= 8
    if variant == "second_pair_sigma":
        return entry == "calibration" and kind == "err" and vec and n_out >= 8
    if variant in ("last_partial_dropped", "partial_stride_1"):
        return fc.n_workgroups(case["rows"]) >= 2
    if variant == "no_reload":
        return passes >= 2
    if variant == "group_first_is_K":
        return passes >= 2 and (entry == "lppd" or kind != "cat")
    if variant == "train_labels":
        return bool(case["train_rows"]) and entry != "uncertainty"
    return bool(case["train_rows"])


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def _phi(u):
    return 0.5 * np.vectorize(math.erfc)(-u / math.sqrt(2.0))


def _vector_reads(z, bug):
    """The values a float4 build reads: z itself, or with every vector past the first replaced by the one before it."""
    if bug != "second_vector_reads_first" or z.shape[2] % 4 or z.shape[2] < 8:
        return z
    zr = z.copy()
    zr[:, :, 4:] = z[:, :, :-4]
    return zr


def _totals(per_row, bug):
    """Quantity q's total from per_row [n_q][n_rows]: partials part[q * n_wg + w] of workgroup w's 256 rows, added in workgroup order."""
    n_q, n = per_row.shape
    n_wg = fc.n_workgroups(n)
    part = np.zeros(n_q * n_wg + n_wg)              # (room behind the partials for the reads of partial_stride_1: zeros)
    for q in range(n_q):
        for w in range(n_wg):
            part[q * n_wg + w] = per_row[q, w * fc.WORKGROUP:(w + 1) * fc.WORKGROUP].sum()
    stride = 1 if bug == "partial_stride_1" else n_wg
    last = n_wg - 1 if bug == "last_partial_dropped" else n_wg
    out = np.zeros(n_q)
    for q in range(n_q):
        for w in range(last):
            out[q] += part[q * stride + w]
    return out


def _first(s0, j, bug):
    return j == 0 if bug == "group_first_is_K" else s0 + j == 0


def _reload(s0, bug):
    return s0 > 0 and bug != "no_reload"


def _lppd(z, labels, kind, sigma, groups, bug):
    n_sets, n, c = z.shape
    zr = _vector_reads(z, bug)
    rows = np.arange(n)
    acc = np.zeros((5, n))                          # m, sum exp(ll - m), K, sum (ll - K), sum (ll - K)^2
    ll_set = np.zeros((n_sets, n))
    for s0, g in groups:
        m, e, k0, s1, s2 = (acc.copy() if _reload(s0, bug) else np.zeros((5, n)))
        for j in range(g):
            s = s0 + j
            if kind == "cat":
                mx = zr[s].max(axis=1)
                se = np.zeros(n)
                for k in range(c):
                    se += np.exp(zr[s][:, k] - mx)
                ll = z[s][rows, labels] - (mx + np.log(se))      # (the label's value is read by its own index, not as a vector)
            else:
                ll = np.zeros(n)
                for k in range(c):
                    u = (labels[:, k] - zr[s][:, k]) * (1.0 / sigma[s, k])
                    ll += (-0.5 * math.log(2 * math.pi) - math.log(sigma[s, k])) - 0.5 * u * u
            ll_set[s] = ll
            if _first(s0, j, bug):
                m, e, k0, s1, s2 = ll.copy(), np.ones(n), ll.copy(), np.zeros(n), np.zeros(n)
            else:
                with np.errstate(over="ignore", invalid="ignore"):
                    up = ll > m
                    e = np.where(up, e * np.exp(m - ll) + 1.0, e + np.exp(ll - m))
                m = np.where(up, ll, m)
                s1 = s1 + (ll - k0)
                s2 = s2 + (ll - k0) ** 2
        acc = np.stack([m, e, k0, s1, s2])
    m, e, k0, s1, s2 = acc
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = m + np.log(e) - math.log(n_sets)
    mean = k0 + s1 / n_sets
    pw = np.maximum(0.0, (s2 - s1 * s1 / n_sets) / (n_sets - 1.0)) if n_sets > 1 else np.zeros(n)
    tot = _totals(np.concatenate([ll_set, np.stack([lp, mean, pw])]), bug)            # [n_sets + 3][n_wg]
    return dict(lppd_i=lp, mean_log_lik_i=mean, p_waic_i=pw, log_lik_sample=tot[:n_sets], lppd=tot[n_sets], mean_log_lik=tot[n_sets + 1],
                p_waic=tot[n_sets + 2])


def _softmax_fold(z, groups, bug):
    """acc [C + 1][n_rows]: the sets' probabilities summed class by class, then the sum of their entropies."""
    n_sets, n, c = z.shape
    vec = c % 4 == 0
    zr = _vector_reads(z, bug)
    acc = np.zeros((c + 1, n))
    for s0, g in groups:
        h = acc[c].copy() if _reload(s0, bug) else np.zeros(n)
        mx, se = [], []
        for j in range(g):
            v = zr[s0 + j]
            top = v.max(axis=1)
            e, ez = np.zeros(n), np.zeros(n)
            for k in range(c):
                d = v[:, k] - top
                e += np.exp(d)
                ez += np.exp(d) * d
            h += np.log(e) - ez / e
            mx.append(top)
            se.append(e)
        acc[c] = h
        for k in range(c):
            slot = k % 4 if (bug == "class_index_drops_k" and vec) else k
            a = acc[slot].copy() if _reload(s0, bug) else np.zeros(n)
            for j in range(g):
                a += np.exp(zr[s0 + j][:, k] - mx[j]) / se[j]
            acc[slot] = a
    return acc


def _uncertainty(z, kind, groups, bug):
    n_sets, n, n_out = z.shape
    if kind == "cat":
        acc = _softmax_fold(z, groups, bug)
        m = acc[:n_out].T / n_sets
        with np.errstate(divide="ignore", invalid="ignore"):
            pe = -np.where(m > 0, m * np.log(m), 0.0).sum(axis=1)
        ee = acc[n_out] / n_sets
        mi = np.maximum(0.0, pe - ee) if n_sets > 1 else np.zeros(n)
        tot = _totals(np.stack([pe, ee, mi]), bug) / n
        return dict(mean_prob=m, predictive_entropy_i=pe, expected_entropy_i=ee, mutual_information_i=mi, predictive_entropy=tot[0], expected_entropy=tot[1],
                    mutual_information=tot[2])
    sp = kind == "err"
    t_n = n_out // 2 if sp else n_out
    zr = _vector_reads(z, bug)
    acc = np.zeros((4, t_n, n))                     # K, sum (mu - K), sum (mu - K)^2, sum sigma^2
    for s0, g in groups:
        for o in range(n_out):
            if o < t_n:
                k0, s1, s2 = acc[:3, o].copy() if _reload(s0, bug) else np.zeros((3, n))
                for j in range(g):
                    mu = zr[s0 + j][:, o]
                    if _first(s0, j, bug):
                        k0 = mu.copy()
                    else:
                        s1 = s1 + (mu - k0)
                        s2 = s2 + (mu - k0) ** 2
                acc[0, o], acc[1, o], acc[2, o] = k0, s1, s2
            else:
                sg = acc[3, o - t_n].copy() if _reload(s0, bug) else np.zeros(n)
                for j in range(g):
                    sg += _softplus(zr[s0 + j][:, o]) ** 2
                acc[3, o - t_n] = sg
    mean = (acc[0] + acc[1] / n_sets).T
    ev = (np.maximum(0.0, (acc[2] - acc[1] * acc[1] / n_sets) / n_sets) if n_sets > 1 else np.zeros((t_n, n))).T
    av = (acc[3] / n_sets).T
    tot = _totals(np.concatenate([mean.T, (ev + av).T, av.T, ev.T]), bug).reshape(4, t_n) / n                  # [4][T][n_wg]
    out = dict(mean=mean, epistemic_var=ev, mean_avg=tot[0], epistemic_var_avg=tot[3])
    if sp:
        out.update(aleatoric_var=av, total_var=ev + av, total_var_avg=tot[1], aleatoric_var_avg=tot[2])
    return out


def _calibration(z, labels, kind, sigma, n_bins, levels, groups, bug):
    n_sets, n, n_out = z.shape
    rows = np.arange(n)
    if kind == "cat":
        m = _softmax_fold(z, groups, bug)[:n_out].T / n_sets
        best = np.argmax(m, axis=1)                  # (the first among equal ones)
        conf = m[rows, best]
        hit = np.zeros((n, n_out))
        hit[rows, labels] = 1.0
        brier = ((m - hit) ** 2).sum(axis=1)
        with np.errstate(divide="ignore"):
            nll = -np.log(m[rows, labels])
        ok = best == labels
        b = np.clip(np.floor(conf * n_bins).astype(np.int64), 0, n_bins - 1)
        count, n_correct = np.bincount(b, minlength=n_bins), np.bincount(b[ok], minlength=n_bins)
        tot = _totals(np.stack([brier, nll, ok.astype(np.float64)] + [np.where(b == q, conf, 0.0) for q in range(n_bins)]), bug)   # [3 + B][n_wg]
        sum_conf = tot[3:]
        full = count > 0
        gaps = np.abs(n_correct[full] / count[full] - sum_conf[full] / count[full])
        return dict(confidence=conf, predicted_class=best, brier_i=brier, nll_i=nll, count=count, sum_confidence=sum_conf, n_correct=n_correct,
                    accuracy=n_correct.sum() / n, brier=tot[0] / n, nll=tot[1] / n, ece=float(np.sum(count[full] / n * gaps)), mce=float(gaps.max()))
    sp = kind == "err"
    vec = n_out % 4 == 0
    t_n = n_out // 2 if sp else n_out
    zr = z if sp else _vector_reads(z, bug)          # (means plus sigmas are read in pairs, never as float4)
    acc = np.zeros((3, t_n, n))                     # K, sum (mu - K), sum Phi
    for s0, g in groups:
        for t in range(t_n):
            k0, s1, ph = acc[:, t].copy() if _reload(s0, bug) else np.zeros((3, n))
            for j in range(g):
                s = s0 + j
                mu = zr[s][:, t]
                if sp:
                    at = t_n + t - 2 if (bug == "second_pair_sigma" and vec and t >= 2) else t_n + t
                    sg = _softplus(z[s][:, at])
                else:
                    sg = sigma[s, t]
                if _first(s0, j, bug):
                    k0 = mu.copy()
                else:
                    s1 = s1 + (mu - k0)
                ph = ph + _phi((labels[:, t] - mu) / sg)
            acc[0, t], acc[1, t], acc[2, t] = k0, s1, ph
    pit = (acc[2] / n_sets).T
    mean = (acc[0] + acc[1] / n_sets).T
    sq = (labels - mean) ** 2
    b = np.clip(np.floor(pit * n_bins).astype(np.int64), 0, n_bins - 1)
    pit_hist = np.stack([np.bincount(b[:, t], minlength=n_bins) for t in range(t_n)])
    covered = np.array([[int(np.sum(np.abs(pit[:, t] - 0.5) <= lv / 2)) for lv in levels] for t in range(t_n)], dtype=np.int64).reshape(t_n, len(levels))
    tot = _totals(np.concatenate([sq.T, pit.T]), bug).reshape(2, t_n)                                          # [2][T][n_wg]
    coverage = covered / n
    return dict(pit=pit, mean=mean, sq_err=sq, pit_hist=pit_hist, covered=covered, rmse=np.sqrt(tot[0] / n), mean_pit=tot[1] / n, coverage=coverage,
                coverage_error=np.mean(np.abs(coverage - np.array(levels)[None, :]), axis=1) if len(levels) else None)


def _pad_rows(v, n_rows, n_done):
    """A per-row array of the first n_done rows with zeros for the rows that were not folded."""
    v = np.asarray(v)
    if v.ndim == 0 or v.shape[0] != n_done:
        return v
    out = np.zeros((n_rows,) + v.shape[1:], dtype=v.dtype)
    out[:n_done] = v
    return out


def model(entry, name, z, bug=None):
    """The model of ``entry`` on a case's pre-output values z [S, N, outputs]; ``bug`` one of VARIANTS or None."""
    inp = fc.inputs(name)
    case, kind, labels, n = inp["case"], inp["kind"], inp["labels"], z.shape[1]
    if bug == "train_labels":
        labels = inp["train_labels"][np.arange(n) % case["train_rows"]]      # (rows past the training slot's: whatever lies there)
    if bug == "train_row_count":
        z, labels = z[:, :case["train_rows"]], labels[:case["train_rows"]]
    if entry == "lppd":
        out = _lppd(z, labels, kind, inp["sigma"], inp["groups"], bug)
    elif entry == "uncertainty":
        out = _uncertainty(z, kind, inp["groups"], bug)
    else:
        out = _calibration(z, labels, kind, inp["sigma"], case["n_bins"], case["levels"], inp["groups"], bug)
    if bug == "train_row_count":
        per_row = {"log_lik_sample"} if entry == "lppd" else set()           # ([n_sets], not a per-row array, whatever its length)
        out = {k: v if (v is None or k in per_row) else _pad_rows(v, n, case["train_rows"]) for k, v in out.items()}
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", PAIRS)
def test_right_model_agrees_and_every_wrong_one_is_far(entry, name):
    case = fc.CASES[name]
    z = fc.oracle_z(name)
    want = fc.want_of(entry, name, z)
    right = model(entry, name, z)
    assert sorted(k for k in right if right[k] is not None) == sorted(k for k in want if want[k] is not None)
    dev = fc.worst_deviation(right, want)
    assert dev <= fc.HOST_TOL, (entry, name, dev)
    if entry != "calibration" or fc.rows_that_may_fall_either_way(name, z) == 0:
        for k in fc.integer_fields(want):
            np.testing.assert_array_equal(right[k], want[k], err_msg="%s %s %s" % (entry, name, k))
    for variant in VARIANTS:
        if applies(variant, entry, case):
            far = fc.worst_deviation(model(entry, name, z, variant), want)
            assert far >= fc.WRONG_FACTOR * fc.TOL[entry], (entry, name, variant, far)


@pytest.mark.parametrize("entry", fc.ENTRIES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_variant_has_a_case_that_catches_it(variant, entry):
    if (variant, entry) in NOT_THIS_ENTRYS:
        assert not any(applies(variant, entry, fc.CASES[n]) for n in fc.cases_of(entry))
        return
    assert any(applies(variant, entry, fc.CASES[n]) for n in fc.cases_of(entry)), (variant, entry)


def test_where_a_variant_does_not_apply_it_is_the_right_fold():
    """``applies`` leaves nothing out by choice: on a case a variant does not apply to, the wrong model IS the right one (checked on the
    one-workgroup, one-vector and one-pass cases of every kind).  Two variants are not asked: with a single workgroup the last partial
    is the only one, and dropping it is a mistake; the test-table variants have no training slot to read from."""
    for name in ("rows_255", "rows_256", "classes_4", "targets_4", "outputs_4", "runs_3_cat", "runs_3_reg", "runs_2_err"):
        z = fc.oracle_z(name)
        for entry in fc.CASES[name]["entries"]:
            right = model(entry, name, z)
            for variant in VARIANTS:
                if applies(variant, entry, fc.CASES[name]) or variant in ("last_partial_dropped", "train_labels", "train_row_count"):
                    continue
                wrong = model(entry, name, z, variant)
                for k in right:
                    assert (right[k] is None and wrong[k] is None) or np.array_equal(right[k], wrong[k]), (name, entry, variant, k)


def test_table_sanity():
    assert len(set(fc.CASES)) == len(fc.CASES) and all(c["name"] == n for n, c in fc.CASES.items())
    assert {fc.n_workgroups(c["rows"]) for c in fc.CASES.values()} == {1, 2, 3, 4}
    assert max(c["rows"] for c in fc.CASES.values()) == 769                 # (no workload sizes)
    # every VEC and non-VEC build of every fold kernel, with two or more iterations of its loop
    reached = {}
    for entry in fc.ENTRIES:
        for name in fc.cases_of(entry):
            kernel, args, iterations = fc.kernel_build(entry, fc.CASES[name])
            reached[(kernel, args)] = max(reached.get((kernel, args), 0), iterations)
    assert sorted(reached) == sorted(fc.BUILDS)
    assert all(v >= 2 for v in reached.values()), reached
    # the groups are the run lengths, S from 1 to 6; the default is four tanh sets in passes of three and one
    assert {fc.CASES[n]["sets"] for n in fc.CASES if fc.CASES[n]["runs"]} == {1, 2, 3, 4, 5, 6}
    for name, case in fc.CASES.items():
        groups = fc.inputs(name)["groups"]
        assert tuple(g for _, g in groups) == (case["runs"] or {4: (3, 1), 6: (3, 3)}[case["sets"]]), name
        assert [s0 for s0, _ in groups] == list(np.cumsum([0] + [g for _, g in groups])[:-1])
    # calibration's parameters ride along: every number of bins with every number of levels on a regression case
    assert {(c["n_bins"], len(c["levels"])) for c in fc.CASES.values() if c["kind"] != "cat"} == {(b, l) for b in (1, 15, 64) for l in (0, 1, 4)}
    assert {c["n_bins"] for c in fc.CASES.values() if c["kind"] == "cat"} == {1, 15, 64}
    # the test table: its own row count, its own labels or targets
    for name in fc.TEST_TABLE:
        inp = fc.inputs(name)
        assert (len(inp["x"]), len(inp["train_x"])) == (513, 300) and not np.array_equal(inp["labels"][:300], inp["train_labels"])
    assert {fc.CASES[n]["kind"] for n in fc.TEST_TABLE} == {"cat", "reg", "err"}
    assert {e: len(fc.cases_of(e)) for e in fc.ENTRIES} == {"lppd": 51, "uncertainty": 65, "calibration": 65}


@pytest.mark.parametrize("name", fc.cases_of("calibration"))
def test_calibration_cap_on_the_reference(name):
    """test_hip_calibration._kernel_check excuses at most 2 rows that may fall either way; on the float64 oracle's values no case has
    one (the table was made so), and the cap is held here, on the reference alone."""
    count = fc.rows_that_may_fall_either_way(name, uc.oracle_values(fc.inputs(name)))
    assert count <= 2, (name, count)
    assert count == 0, (name, count)


def test_degenerate_single_class():
    """One class: every log-likelihood is 0, every entropy 0, every confidence 1."""
    z = fc.oracle_z("classes_1")
    assert not fc.want_of("lppd", "classes_1", z)["lppd_i"].any()
    u = fc.want_of("uncertainty", "classes_1", z)
    assert not u["predictive_entropy_i"].any() and not u["expected_entropy_i"].any() and np.all(u["mean_prob"] == 1.0)
    assert np.all(fc.want_of("calibration", "classes_1", z)["confidence"] == 1.0)
