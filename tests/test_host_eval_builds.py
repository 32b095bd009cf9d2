"""CPU: the case table of tests/test_hip_chain_oracle.py keeps up with the eval_kernel builds.

Every npbnn_eval_inst_*.hip file sets NPBNN_INST_* and includes npbnn_eval_inst.inc, which emits one eval_kernel instantiation per
first-layer tile count (MT0) its preprocessor conditions keep.  This test reads those defines, runs the .inc's conditionals for each
file, and requires every (MTI, D, LK, FAST, SPEC, CHAIN, BLK, MT0) it emits to be claimed by a case of the GPU table or listed there as
unreachable with a reason - so a new instantiation file, or a new MT0 case, fails here until a GPU test reaches it.  The GPU module is
imported only for its tables: its ``pytestmark`` does not stop an import."""
import glob
import os
import re

import numpy as np

import test_hip_chain_oracle as gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "npbnn_amd", "csrc")
_BOOL = {"true": 1, "false": 0}


def _value(tok, macros):
    tok = tok.strip()
    tok = macros.get(tok, tok)
    return _BOOL.get(tok, tok)


def _eval(expr, macros):
    """A preprocessor condition of the forms the .inc uses: NAME, NAME <op> number, joined by && / ||."""
    py = re.sub(r"[A-Za-z_]\w*", lambda m: str(_value(m.group(0), macros)), expr)
    py = py.replace("&&", " and ").replace("||", " or ").replace("!", " not ").replace(" not =", "!=")
    return bool(eval(py, {}, {}))


def defines(path):
    out = {}
    for line in open(path):
        m = re.match(r"\s*#define\s+(NPBNN_INST_\w+)\s+(\S+)", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def emitted_builds(macros):
    """The (MTI, D, LK, FAST, SPEC, CHAIN, BLK, MT0) instantiations npbnn_eval_inst.inc emits under ``macros``."""
    macros = dict(macros)
    stack, builds, blk = [], set(), 0
    for raw in open(os.path.join(CSRC, "npbnn_eval_inst.inc")):
        line = raw.split("//")[0].strip()
        live = all(stack)
        if line.startswith("#ifndef"):
            stack.append(line.split()[1] not in macros)
        elif line.startswith("#ifdef"):
            stack.append(line.split()[1] in macros)
        elif line.startswith("#if"):
            stack.append(_eval(line[3:], macros))
        elif line.startswith("#else"):
            stack[-1] = not stack[-1]
        elif line.startswith("#endif"):
            stack.pop()
        elif not live:
            continue
        elif line.startswith("#define"):
            parts = line.split()
            macros.setdefault(parts[1], parts[2] if len(parts) > 2 else "1")
        elif "pick_blk" in line and "static" in line:
            blk = 1
        elif "pick_mt0" in line and "static" in line:
            blk = 0
        else:
            m = re.match(r"(?:case\s+(\d+)|default)\s*:\s*return\s+eval_kernel<(\d+)", line)
            if m:
                mt0 = int(m.group(2))
                assert m.group(1) is None or int(m.group(1)) == mt0, line
                key = tuple(int(_value(macros[k], macros)) for k in
                            ("NPBNN_INST_MTI", "NPBNN_INST_D", "NPBNN_INST_LK", "NPBNN_INST_FAST", "NPBNN_INST_SPEC", "NPBNN_INST_CHAIN"))
                builds.add(key + (blk, mt0))
    assert not stack, "unbalanced conditionals in npbnn_eval_inst.inc"
    return builds


def all_builds():
    files = sorted(glob.glob(os.path.join(CSRC, "npbnn_eval_inst_*.hip")))
    assert files
    out = {}
    for path in files:
        d = defines(path)
        assert "NPBNN_INST_NAME" in d and "NPBNN_INST_MTI" in d, path
        for b in emitted_builds(d):
            out.setdefault(b, []).append(os.path.basename(path))
    return out


def test_every_instantiated_build_has_a_case():
    builds = all_builds()
    claimed = {c["key"] for c in gpu.CASES}
    unreachable = {b for b, reason in gpu.UNREACHABLE}
    assert all(reason.strip() for _, reason in gpu.UNREACHABLE)
    missing = sorted(set(builds) - claimed - unreachable)
    assert not missing, "builds no case of test_hip_chain_oracle.CASES reaches: %s" % [(b, builds[b]) for b in missing]
    stale = sorted((claimed | unreachable) - set(builds))
    assert not stale, "cases name builds no instantiation file emits: %s" % stale
    assert not claimed & unreachable


def test_the_parser_sees_the_known_limits():
    """Spot checks of the .inc's rules as the parser reads them: no three-candidate build from three output tiles on
    (max_cand_for), fast builds up to kFastMaxMT0 = 4 tiles, no block-structured spec build, the default case is MT0 8."""
    b = all_builds()
    assert (1, 3, 0, 0, 0, 1, 0, 2) in b and (1, 3, 0, 0, 0, 1, 0, 3) not in b
    assert (1, 2, 0, 0, 0, 1, 0, 8) in b and (1, 1, 2, 0, 0, 1, 0, 8) in b
    assert (1, 1, 0, 1, 0, 1, 0, 4) in b and (1, 1, 0, 1, 0, 1, 0, 5) not in b
    assert (1, 1, 0, 1, 0, 1, 1, 2) in b and (1, 1, 0, 1, 0, 1, 1, 1) not in b
    assert not any(k[4] and k[6] for k in b)
    assert (1, 1, 0, 1, 0, 0, 0, 1) in b                      # the plain-evaluation builds (CHAIN false)
    assert len({k[:6] for k in b}) == len(glob.glob(os.path.join(CSRC, "npbnn_eval_inst_*.hip")))


def test_a_new_instantiation_file_is_caught(tmp_path, monkeypatch):
    """A define file the table does not know (here: a two-candidate row-wise group) shows up as missing builds."""
    src = tmp_path / "csrc"
    src.mkdir()
    for p in glob.glob(os.path.join(CSRC, "npbnn_eval_inst*")):
        (src / os.path.basename(p)).write_text(open(p).read())
    (src / "npbnn_eval_inst_d2_gen.hip").write_text("#define NPBNN_INST_NAME pick_eval_d2_gen\n#define NPBNN_INST_MTI 1\n"
                                                   "#define NPBNN_INST_D 2\n#define NPBNN_INST_LK 2\n#include \"npbnn_eval_inst.inc\"\n")
    monkeypatch.setattr(__import__(__name__), "CSRC", str(src))
    extra = set(all_builds()) - {c["key"] for c in gpu.CASES}
    assert extra and all(k[1] == 2 and k[2] == 2 for k in extra)


def test_state_check_agrees_with_the_float64_stand_in():
    """The GPU module's state check and dispatch driver, run on the float64 stand-in of the device chain: exact agreement for each
    likelihood class and the block-structured first layer, so a GPU failure is the kernel's, not the helper's."""
    import npbnn_amd as bn
    import oracle_backend as ob
    for lik, widths, blocks in (("cat", (29, 7), 0), ("gauss", (13, 40), 0), ("pois", (16, 6), 0), ("cat", (32, 6), 4)):
        ob.serve_from_oracle(lambda b, lik=lik: ob.OracleChainBackend(b, out_kind=0 if lik == "cat" else 1))
        dat = gpu.make_data(lik, 200, 64 if blocks else 12, n_test=40 if lik == "cat" else 0)
        bnn, mcmc = gpu.make_chain(bn, lik, dat, widths, mask_blocks=blocks)
        mcmc.SUB_BATCH = 16
        errs = [gpu.check_state(lik, bnn, mcmc)]
        dec = gpu.drive(lik, bnn, mcmc, 80, worst=errs, accuracy_every=1)
        assert max(errs) == 0.0 and 0 < sum(dec) < 80
        assert gpu.dispatch_sizes(80) and all(7 <= k <= 40 for k in gpu.dispatch_sizes(400, seed=3)[:-1])
        if blocks:
            assert all(np.all(w[m == 0] == 0) for w, m in zip(bnn._w_layers, bnn._mask))
