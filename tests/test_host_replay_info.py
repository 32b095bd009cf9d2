"""NPBNN_INFO_REPLAY_PASSES / _MAX_GROUP: the header's values are the Python constants, and HipContext reads them as a pair."""
import os
import re

from npbnn_amd import _capi as capi
from npbnn_amd.backend import HipContext

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "npbnn_hip.h")


def _enum_values():
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    return {name: int(value) for name, value in re.findall(r"\b(NPBNN_INFO_\w+)\s*=\s*(\d+)", text)}


def test_header_and_python_constants_agree():
    values = _enum_values()
    assert values["NPBNN_INFO_REPLAY_PASSES"] == capi.INFO_REPLAY_PASSES == 22
    assert values["NPBNN_INFO_REPLAY_MAX_GROUP"] == capi.INFO_REPLAY_MAX_GROUP == 23
    assert len(set(values.values())) == len(values)              # (no two info values share a number)


def test_context_reads_them_as_a_pair():
    assert callable(HipContext.replay_info)

    class Stub:
        def info(self, what):
            return {capi.INFO_REPLAY_PASSES: 34, capi.INFO_REPLAY_MAX_GROUP: 3}[what]

    assert HipContext.replay_info(Stub()) == (34, 3)
