"""CPU: the HIP library owns its memory through one buffer type.

Every device or page-locked host allocation the library keeps is a Buffer (npbnn_amd/csrc/npbnn_buf.hip.h), freed by its destructor
or reset().  The allocator's own calls may appear only in that header and in npbnn_pinned_alloc / npbnn_pinned_free (memory handed
to the caller).  The matrices that contexts share (npbnn_share_data) are buffers too, in a store held through a shared_ptr: no
context points into another, counts its users or outlives its own destruction for them.  A new raw owner fails here."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "npbnn_amd", "csrc")
ALLOC = re.compile(r"\b(hipMalloc|hipHostMalloc|hipFree|hipHostFree)\b")
BUFFER_HEADER = "npbnn_buf.hip.h"
PINNED_ENTRIES = ("npbnn_pinned_alloc", "npbnn_pinned_free")


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".c")))


def function_of(lines, i):
    """Name of the C function whose body holds line i (the last line before it that opens one at column 0)."""
    for j in range(i, -1, -1):
        m = re.match(r"[A-Za-z_][\w\s\*:<>,]*?\b(\w+)\(", lines[j])
        if m and not lines[j].startswith((" ", "\t", "#", "//", "}")):
            return m.group(1)
    return None


def test_allocator_calls_only_where_allowed():
    stray = []
    for f in sources():
        if f == BUFFER_HEADER:
            continue
        lines = open(os.path.join(CSRC, f)).read().split("\n")
        for i, line in enumerate(lines):
            code = line.split("//")[0]
            if not ALLOC.search(code):
                continue
            if function_of(lines, i) in PINNED_ENTRIES:
                continue
            stray.append("%s:%d: %s" % (f, i + 1, line.strip()))
    assert not stray, "raw allocator calls outside the buffer type:\n" + "\n".join(stray)


def test_buffer_header_allocates():
    text = open(os.path.join(CSRC, BUFFER_HEADER)).read()
    for call in ("hipMalloc", "hipHostMalloc", "hipFree", "hipHostFree"):
        assert call in text


def test_context_keeps_no_capacity_fields():
    """Each buffer carries its own capacity: no hand-kept *_cap companion in the context or the communicator."""
    for f, name in (("npbnn_ctx.hip.h", "npbnn_ctx"), ("npbnn_comm.hip", "npbnn_comm")):
        m = re.search(r"^struct %s\b[^{]*\{(.*?)^\};" % name, open(os.path.join(CSRC, f)).read(), re.S | re.M)
        assert m, name
        assert not re.search(r"\b\w+_cap\b|\bcap_\w+\b|\bpartial_waves\b", m.group(1)), name


def struct_body(name):
    m = re.search(r"^struct %s\b[^{]*\{(.*?)^\};" % name, open(os.path.join(CSRC, "npbnn_ctx.hip.h")).read(), re.S | re.M)
    assert m, name
    return "\n".join(line.split("//")[0] for line in m.group(1).split("\n"))


def test_shared_matrices_have_no_hand_kept_ownership():
    """The matrices and scales that npbnn_share_data shares live in one store owned through a shared_ptr: the context and its tables
    keep no owner pointer, user count, lingering state or borrowed flag, and no raw float pointer to a matrix or a scale."""
    ctx, dataset = struct_body("npbnn_ctx"), struct_body("Dataset")
    assert not re.search(r"\b(data_owner|n_borrowers|zombie)\b", ctx)
    assert not re.search(r"\b(borrowed|x16w_borrowed)\b", dataset)
    for body in (ctx, dataset):
        assert not re.search(r"\bfloat\s*\*\s*(X|X16|X16w|d_xscale|d_wscale|xscale|wscale)\b", body)
    assert re.search(r"\bstd::shared_ptr<\s*FeatureStore\s*>", ctx)
    store = struct_body("FeatureStore") + struct_body("FeatureTable")
    for member in ("X", "X16", "X16w", "xscale", "wscale"):
        assert re.search(r"\bDevBuf<float>[^;]*\b%s\b" % member, store), member
