"""bench.py's two kinds of run: a plain one does only what its headline needs (set-up, warm-up, the timed steps, --dump-outputs, the
line); --full adds the legs that take runs of their own (roofline, CPU baseline, parity, the other configurations, the row-sharded
chain).  The CPU tests drive ``report`` on stand-ins; the GPU tests run the script end to end."""
import json
import os
import subprocess
import sys
import types

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


class _Ctx:
    sync_fallbacks = 0

    def l0_mode(self):
        return "f16-split"

    def info(self, what):
        return 0


class _Mcmc:
    def __init__(self):
        self._backend = types.SimpleNamespace(ctx=_Ctx(), close=lambda: None)
        self._device_passes, self._device_void_passes, self._device_iterations, self._device_accepted = 900, 0, 2000, 50
        self._device_schedule_used, self._acceptance_rate, self._logLik = 4, 0.02, -230000.0


def _args(*argv):
    old = sys.argv
    sys.argv = ["bench.py"] + list(argv)
    try:
        return bench.parse_args()
    finally:
        sys.argv = old


def _report(args, cand=3):
    wl = types.SimpleNamespace(description="stand-in workload")
    book = dict(acc=0, passes=0, voids=0, its=0)
    return bench.report(args, wl, None, _Mcmc(), 1, 0.02, args.steps * bench.ITERATIONS_PER_STEP, book, "none", 1, False, cand)


def test_full_is_off_by_default():
    assert _args().full is False
    assert _args("--full").full is True


def test_plain_report_runs_nothing_beyond_the_headline(monkeypatch):
    def must_not_run(*a, **k):
        raise AssertionError("a plain run started a leg of --full")
    for name in ("kernel_roofline", "cpu_baseline", "moving_chain", "other_config", "wide_config", "wide_fused_config", "group_pass_leg",
                 "row_sharded_chain"):
        monkeypatch.setattr(bench, name, must_not_run)
    line = _report(_args("--steps", "20", "--warmup", "5"), cand=3)
    for key in HEADLINE:
        assert key in line
    assert line["value"] == pytest.approx(20 * bench.ITERATIONS_PER_STEP / 0.02) and line["ms_per_step"] == pytest.approx(1.0)
    assert line["higher_is_better"] is True and line["dtype"] == "f16x3-split/f32"
    assert line["config"]["candidates_per_pass"] == 3 and line["cpu_baseline"] is None
    assert "roofline" not in line and "other_configs" not in line and "parity" not in line
    assert len(json.dumps(line)) < 4096


def test_full_report_adds_the_roofline(monkeypatch):
    monkeypatch.setattr(bench, "kernel_roofline", lambda *a, **k: ({"frac": 0.5}, 2))
    line = _report(_args("--full", "--no-cpu-baseline", "--steps", "20"), cand=None)
    assert line["roofline"] == {"frac": 0.5} and line["config"]["candidates_per_pass"] == 2
    for key in HEADLINE:
        assert key in line


def _run_bench(*argv, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_and_full_runs_on_the_gpu(tmp_path):
    """A plain run prints the headline and writes its dump; --full (config 2 alone, no CPU baseline) adds the roofline of the same
    pass kernel and describes the chain the same way."""
    plain = _run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for key in HEADLINE:
        assert key in plain
    assert plain["value"] > 0 and plain["config"]["candidates_per_pass"] >= 1
    assert "roofline" not in plain and "other_configs" not in plain and plain["cpu_baseline"] is None
    assert os.path.exists(os.path.join(str(tmp_path), "predictions.npy"))
    assert os.path.exists(os.path.join(str(tmp_path), "chain_scalars.npy"))
    full = _run_bench("--steps", "3", "--warmup", "1", "--full", "--only", "--no-cpu-baseline")
    assert full["roofline"]["kernel_ms"] > 0
    assert full["config"]["candidates_per_pass"] == plain["config"]["candidates_per_pass"]
    assert full["dtype"] == plain["dtype"] and full["config"]["layer0"] == plain["config"]["layer0"]
