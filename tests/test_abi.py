"""CPU-side checks of the C-ABI library: it builds for gfx950, loads, and exports every symbol include/hamgnn_hip.h declares; and of the typed call
of hamgnn_amd/_lib.py, which takes its signatures from that header (CPU tensors and NULLs only: no call here reaches a launch)."""
import os
import re

from hamgnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_loads_and_exports_header_symbols():
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "hamgnn_hip.h")).read()
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    assert L.hg_version() >= 1


def test_parsed_prototypes_are_the_exports_and_the_loaded_symbols():
    L = _lib.lib()
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert set(protos) == set(_lib.EXPORTS) == set(_lib._bound) and len(protos) == len(_lib.EXPORTS)
    assert all(hasattr(L, name) for name in protos)
    assert protos["hg_add_rows"] == ("int", [("const float*", "a"), ("int64_t", "sa"), ("const float*", "b"), ("int64_t", "sb"), ("const float*", "c"), ("int64_t", "sc"),
                                             ("int64_t", "rows"), ("int", "D"), ("float*", "out"), ("int64_t", "so"), ("void*", "stream")])
    assert protos["hg_last_error"] == ("const char*", []) and protos["hg_scratch_bytes"][0] == "int64_t"
    assert L.hg_add_rows.argtypes is None                      # the raw handle stays untyped


def test_parser_refuses_an_unknown_type_spelling():
    import pytest
    text = open(_lib.HEADER_PATH).read()
    for bad in ("unsigned", "const int16_t*", "float**"):
        with pytest.raises(ValueError, match="unknown type spelling"):
            _lib.parse_header(text.replace("int hg_add_rows(const float* a, int64_t sa", f"int hg_add_rows(const float* a, {bad} sa"))


def test_host_arrays_come_from_the_header():
    text = open(_lib.HEADER_PATH).read()
    protos = _lib.parse_header(text)
    is_host = _lib.host_arrays(text, protos)
    host = {n for _, ps in protos.values() for t, n in ps if is_host(t, n)}
    assert host == {"src", "src_stride", "wig_off", "dims", "part_table_host", "consts_host", "src_idx"}
    assert not is_host("const int64_t*", "src")                # hg_attn_logits' sender index is a device tensor


def test_typed_call_checks_every_argument_before_the_library_is_reached():
    import numpy as np, pytest, torch
    from hamgnn_amd import ops
    call, strided = _lib.call, _lib.strided
    f = torch.zeros(4, 6)
    slots = (("a", None), ("sa", 6), ("b", None), ("sb", 6), ("c", None), ("sc", 0), ("rows", 4), ("D", 6), ("out", None), ("so", 6))      # every tensor but the one under test NULL
    add = lambda **kw: call("hg_add_rows", *[kw.get(k, d) for k, d in slots])
    with pytest.raises(TypeError, match="hg_add_rows takes 10 arguments"):
        call("hg_add_rows", f, 6)
    with pytest.raises(ValueError, match="hg_segment_sum: perm .*int64"):
        call("hg_segment_sum", None, 8, None, torch.zeros(5, dtype=torch.int32), 3, 8, None, 8)
    with pytest.raises(ValueError, match="hg_add_rows: b .*float32"):
        add(b=f.double())
    with pytest.raises(ValueError, match="hg_add_rows: a must be contiguous"):
        add(a=torch.zeros(6, 4).t())
    with pytest.raises(ValueError, match="hg_add_rows: a: strided"):
        add(a=strided(torch.zeros(6, 4).t()))
    with pytest.raises(ValueError, match="hg_radial_hidden: dims is a host array"):
        call("hg_radial_hidden", None, 0, None, torch.zeros(3, dtype=torch.int32), 2, 1.0, None)
    with pytest.raises(ValueError, match="hg_radial_hidden: dims is a host array"):
        call("hg_radial_hidden", None, 0, None, np.zeros(3, np.int64), 2, 1.0, None)
    tp = lambda src: call("hg_tp_fused", src, None, 1, *[None] * 2, 64, None, 0, None, *[None] * 2, 0, *[None] * 2, 8, 0, 0, 0, None, 0, None, 0)
    with pytest.raises(ValueError, match=r"hg_tp_fused: src\[.\] .*float32"):      # an array of pointers from its tensors: each checked as a strided() one
        tp([f.double(), None, None, None])
    with pytest.raises(ValueError, match=r"hg_tp_fused: src\[.\]: strided"):
        tp([torch.zeros(6, 4).t()])
    with pytest.raises(RuntimeError, match="needs CUDA"):
        tp([None, torch.zeros(4, 12)[:, 3:9]])
    with pytest.raises(ValueError, match="hg_tp_fused: src is a host array"):
        tp(f)
    with pytest.raises(ValueError, match="hg_add_rows: out .*device pointer"):
        add(out=np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="hg_add_rows: D = 2147483648 does not fit int"):
        add(D=2 ** 31)
    with pytest.raises(ValueError, match="hg_add_rows: rows"):
        add(rows=2 ** 63)
    with pytest.raises(TypeError, match="hg_add_rows: D .*integer"):
        add(D=6.0)
    with pytest.raises(TypeError, match="hg_add_rows: sa"):
        add(sa=torch.zeros(()))
    with pytest.raises(TypeError, match="hg_dos_broaden: sigma"):
        call("hg_dos_broaden", None, None, 5, 0, 0.0, 0.1, 10, "0.1", 0, None)
    with pytest.raises(TypeError, match="hg_scratch_bytes: entry_point"):
        call("hg_scratch_bytes", "hg_edge_geometry", 1, 0)
    # a CPU tensor of the right type and layout gets as far as the device check, the last one: _require_gpu's own error, unchanged
    with pytest.raises(RuntimeError) as want:
        ops._require_gpu(f)
    with pytest.raises(RuntimeError) as got:
        add(out=f)
    assert str(got.value) == str(want.value) and "hg_add_rows" not in str(got.value)
    with pytest.raises(RuntimeError, match="needs CUDA"):
        add(a=strided(torch.zeros(4, 12)[:, 3:9]), sa=12)         # a column slice passes the contiguity rule as strided()
    with pytest.raises(ValueError, match="hg_add_rows: a must be contiguous"):
        add(a=torch.zeros(4, 12)[:, 3:9], sa=12)


def test_typed_call_puts_the_values_into_the_right_slots():
    """the NULL cases that tests/test_dos_cpu.py pins on the raw handle, through the typed call: none can reach a launch"""
    import numpy as np, pytest
    call = _lib.call
    assert call("hg_dos_broaden", None, None, 5, 0, 0.0, 0.1, 10, 0.1, 0, None) is None                    # no column
    assert call("hg_dos_broaden", None, None, np.int64(5), True, 0, np.float32(0.5), 0, 0.1, False, None) is None      # no energy; numpy scalars and bools
    for bad in (dict(sigma=0.0), dict(dE=-0.1), dict(ns=-1), dict()):                                      # the last: good sizes, NULL tensors
        a = dict(ns=5, Gp=4, E0=0.0, dE=0.1, ne=10, sigma=0.1)
        a.update(bad)
        with pytest.raises(RuntimeError, match="hg_dos_broaden"):
            call("hg_dos_broaden", None, None, a["ns"], a["Gp"], a["E0"], a["dE"], a["ne"], a["sigma"], 0, None)
    assert call("hg_mulliken_weights", None, None, 0, 4, None, None, 1, 2, None, None) is None             # no state
    with pytest.raises(RuntimeError, match="hg_mulliken_weights"):
        call("hg_mulliken_weights", None, None, 3, 4, None, None, 2, 2, None, None)                        # Gp < 1 + G
    with pytest.raises(RuntimeError, match="hg_mulliken_weights"):
        call("hg_mulliken_weights", None, None, 3, 0, None, None, 0, 1, None, None)                        # M = 0
    assert call("hg_mulliken_weights", None, None, 0, 4, None, None, 1, 2, None, None, stream=0) is None
    assert call("hg_version") >= 1 and call("hg_build_config", 7) == -1
    assert call("hg_scratch_bytes", b"hg_edge_geometry", 822350, 0) == 822350 * 16 and call("hg_scratch_bytes", None, 1, 0) == -1


def test_product_does_not_import_oracle():
    import subprocess, sys
    code = "import sys; import hamgnn_amd, hamgnn_amd.models.hamgnn_conv, hamgnn_amd.models.hamgnn_output; assert not any(m.startswith('oracle') for m in sys.modules)"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "hamgnn_amd")):
        for fn in files:
            if fn.endswith(".py"):
                src = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), fn


def test_missing_gpu_fails_loudly():
    import pytest, torch
    from hamgnn_amd import ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        ops._require_gpu(torch.zeros(1))


def test_scratch_query_is_host_only_and_matches_the_documented_sizes():
    """hg_scratch_bytes: the workspace query of the boundary (no entry point allocates); callable without a GPU"""
    import ctypes as C
    L = _lib.lib()
    L.hg_scratch_bytes.restype = C.c_int64
    L.hg_scratch_bytes.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    assert L.hg_scratch_bytes(b"hg_edge_geometry", 822350, 0) == 822350 * 16          # ang_scratch [E][4] floats
    assert L.hg_scratch_bytes(b"hg_zero_point_shift", 1, 256) == 2 * 256 * 8            # partial_scratch [2 nparts] doubles
    assert all(L.hg_scratch_bytes(n.encode(), 1000, 0) == 0 for n in _lib.EXPORTS if n not in ("hg_edge_geometry", "hg_zero_point_shift"))
    assert L.hg_scratch_bytes(None, 1, 0) == -1 and L.hg_scratch_bytes(b"hg_tp_is", -1, 0) == -1
