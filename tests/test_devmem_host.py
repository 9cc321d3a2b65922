"""Device and pinned memory have one owner type (mega-nerf-viewer_amd/csrc/mnv_devmem.h): no other source file allocates or frees by
hand, and the private grow-only helpers that file replaced have not come back.  Reads the sources only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mega-nerf-viewer_amd")
OWNER = os.path.join(PKG, "csrc", "mnv_devmem.h")
CLOCKS_LINE = "if (!clocks) (void)hipMalloc((void **)&clocks, 128);"   # mnv_mlp.hip, -DMNV_MLP_CLOCKS measurement variant only


def _sources():
    files = []
    for sub, pats in ((os.path.join(PKG, "csrc"), ("*.h", "*.hip", "*.cpp")), (os.path.join(PKG, "host"), ("*.hpp", "*.cpp")),
                      (os.path.join(ROOT, "include"), ("*.h", "*.hpp"))):
        for p in pats:
            files += glob.glob(os.path.join(sub, p))
    assert len(files) > 50 and OWNER in files
    return sorted(files)


def _code_lines(path):
    """(line number, text) of a file with // comments and string literals blanked: the error texts name hipMalloc(...) on purpose."""
    out = []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = re.sub(r'"(?:\\.|[^"\\])*"', '""', line)
            out.append((no, line.split("//", 1)[0]))
    return out


def _calls(name):
    """{file: [line numbers]} of calls of `name` outside the owner header."""
    hits = {}
    for path in _sources():
        if path == OWNER:
            continue
        nos = [no for no, text in _code_lines(path) if re.search(r"\b" + name + r"\s*\(", text)]
        if nos:
            hits[os.path.relpath(path, PKG)] = nos
    return hits


def test_raw_allocation_calls_live_in_the_owner_header_only():
    owner = "".join(t for _, t in _code_lines(OWNER))
    for name in ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"):
        assert re.search(r"\b" + name + r"\s*\(", owner), name
    assert _calls("hipFree") == {} and _calls("hipHostMalloc") == {} and _calls("hipHostFree") == {}
    # the single named exception: the phase clocks of the MLP's measurement variant (never freed, never built into the library)
    hits = _calls("hipMalloc")
    assert list(hits) == [os.path.join("csrc", "mnv_mlp.hip")] and len(hits[os.path.join("csrc", "mnv_mlp.hip")]) == 1, hits
    with open(os.path.join(PKG, "csrc", "mnv_mlp.hip"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    no = hits[os.path.join("csrc", "mnv_mlp.hip")][0]
    assert lines[no - 1].strip() == CLOCKS_LINE
    assert any(l.strip() == "#ifdef MNV_MLP_CLOCKS" for l in lines[no - 4:no - 1])


def test_stream_ordered_scratch_stays_in_the_reference_layout_march():
    for name in ("hipMallocAsync", "hipFreeAsync"):
        assert list(_calls(name)) == [os.path.join("csrc", "mnv_march_ref_layout.hip")], name


def test_private_grow_helpers_are_gone():
    text = {os.path.relpath(p, PKG): "\n".join(t for _, t in _code_lines(p)) for p in _sources()}
    everything = "\n".join(text.values())
    assert not re.search(r"\bDeviceBuffer\b", everything)
    assert not re.search(r"\bregrow\b", everything)
    assert not re.search(r"\bstruct\s+Workspace\b", everything)
    # one grow(): the owner header's
    defs = {f: len(re.findall(r"^\s*(?:static\s+|inline\s+)*(?:int|hipError_t)\s+grow\s*\(", t, re.M)) for f, t in text.items()}
    assert {f: n for f, n in defs.items() if n} == {os.path.join("csrc", "mnv_devmem.h"): 1}, defs
    # ws_reserve keeps its name and goes through it
    refine = text[os.path.join("csrc", "mnv_refine.hip")]
    body = refine[refine.index("int ws_reserve("):]
    body = body[:body.index("\n}\n")]
    assert "grow(g_ws[dev]" in body and ".alloc(" not in body
    # the handles keep no capacity beside the pointer
    for f, word in ((os.path.join("csrc", "mnv_accel.h"), "patch_prefix_words"), (os.path.join("csrc", "mnv_mlp.h"), "scratch_bytes"),
                    (os.path.join("csrc", "mnv_wireframe.hip"), "cap_list"), (os.path.join("csrc", "mnv_mesh.hip"), "cap_list")):
        assert word not in text[f], (f, word)


def test_the_live_byte_accessor_is_a_test_hook():
    with open(os.path.join(PKG, "csrc", "mnv_probe.hip"), encoding="utf-8") as f:
        assert "mnv_hook_live_bytes" in f.read()
    for path in _sources():
        if not path.endswith("mnv_probe.hip"):
            with open(path, encoding="utf-8") as f:
                assert "int64_t mnv_hook_live_bytes" not in f.read(), path
