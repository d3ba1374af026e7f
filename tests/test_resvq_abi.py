"""include/crane_gpu_resv/resv_probe.h: the library exports what the header declares, the binding names the same calls, the ctypes
mirrors have the header's fields in the header's order, and the pinned ABI 4 directory is as it was."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_resv", "resv_probe.h")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.RESVQ_ABI_SYMBOLS) == ["cns_resvq_run", "cns_resvq_set_state", "cns_resvq_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in resv_probe.h but not exported"


def test_shape_signature_follows_the_header():
    from cranesched_amd import abi
    m = re.search(r"\bint cns_resvq_shape\(([^)]*)\);", _source())
    assert m, "cns_resvq_shape is not declared as returning int"
    params = [p.strip() for p in m.group(1).split(",")]
    assert all(p.startswith("uint32_t* ") for p in params), params
    assert tuple(p.split()[-1] for p in params) == abi.ResvqShape._fields == ("pick_block", "pick_grid", "sort_tile", "scan_span")


def test_shape_without_a_handle(built):
    """No handle, no GPU; null pointers are allowed one by one and all at once; the values are those of the gate's and the sorter's
    own constants and are what the kernels' layout needs (whole waves, a power-of-two tile of whole blocks)."""
    from cranesched_amd import engine
    L = engine.lib()
    v = [C.c_uint32(0) for _ in range(4)]
    assert L.cns_resvq_shape(*[C.byref(x) for x in v]) == 0
    shape = engine.resvq_shape()
    assert tuple(x.value for x in v) == tuple(shape) == (256, 256, 4096, 256)
    assert L.cns_resvq_shape(None, None, None, None) == 0
    for skip in range(4):
        w = [C.c_uint32(77) for _ in range(4)]
        assert L.cns_resvq_shape(*[None if i == skip else C.byref(x) for i, x in enumerate(w)]) == 0
        assert [x.value for x in w] == [77 if i == skip else shape[i] for i in range(4)]
    assert shape.pick_block % 64 == 0 and shape.pick_grid >= 1 and shape.sort_tile % shape.pick_block == 0 and shape.scan_span >= 64
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.cns_gate_shape(C.byref(a), C.byref(b), C.byref(c)) == 0 and c.value == shape.scan_span   # one scan kernel serves both


def test_struct_mirrors_follow_the_header():
    from cranesched_amd import abi
    src = _source()
    for cname, mirror in (("cns_resvq_soa", abi.CnsResvqSoa), ("cns_resvq_out", abi.CnsResvqOut)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", src, flags=re.S).group(1)
        fields = re.findall(r"([A-Za-z_0-9 ]+?)(\*?)\s*\b([a-z_]+);", body)
        assert [f[2] for f in fields] == [f[0] for f in mirror._fields_], cname
        for (ctype, star, name), (_, py) in zip(fields, mirror._fields_):
            assert py is (C.c_void_p if star else C.c_uint64), f"{cname}.{name}: {ctype.strip()}{star}"
        assert C.sizeof(mirror) == 8 * len(fields)
    assert (abi.RESVQ_OK, abi.RESVQ_NOT_ENOUGH, abi.RESVQ_IN_THE_PAST) == (0, 1, 2)
    assert (abi.RESVQ_FREE, abi.RESVQ_RUNNING, abi.RESVQ_RESERVED, abi.RESVQ_NOT_FOUND) == (0, 1, 2, 3)
    for name, val in re.findall(r"\b(CNS_RESVQ_[A-Z_]+) = (\d+)", src):
        assert getattr(abi, name[4:]) == int(val), name


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "resvq" not in src
