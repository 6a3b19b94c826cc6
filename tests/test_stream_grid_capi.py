"""CPU-side checks of the persistent kernels' grid hook (srcdsp_stream_*):
exported, in the ctypes signature table and the header, marked as an
extension; the Python face; the counters' call skips null pointers; the setter
refuses a negative cap and takes one and zero -- no GPU here."""
import ctypes as C
import os

import pytest

NEW = ("srcdsp_stream_set_grid_cap", "srcdsp_stream_get_grid_cap", "srcdsp_stream_grid_stats")


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_new_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert capi.SIGNATURES["srcdsp_stream_set_grid_cap"] == (C.c_int, [C.c_long])
    assert capi.SIGNATURES["srcdsp_stream_get_grid_cap"] == (C.c_long, [])
    assert len(capi.SIGNATURES["srcdsp_stream_grid_stats"][1]) == 2


def test_header_marks_the_extension(capi):
    with open(capi.HEADER) as f:
        text = f.read()
    for s in NEW:
        at = text.index(" " + s + "(")
        at = text.rindex("SRCDSP_API", 0, at)
        start = text.rindex("/*", 0, at)
        # the comment ends right in front of the declaration and opens with the mark
        assert text.rindex("*/", 0, at) > start and not text[text.rindex("*/", 0, at) + 2:at].strip(), s
        assert text[start:at].startswith("/* Extension"), s
    doc = text[text.rindex("/*", 0, text.index("SRCDSP_API int srcdsp_stream_set_grid_cap(")):]
    doc = doc[:doc.index("*/")]
    # what it is for, what puts the product grids back, and that results do not move
    for word in ("cap >= 1", "0 puts the product", "negative is SRCDSP_ERR_ARG", "Process-wide", "Results do not"):
        assert word in doc, word
    for cite in ("dnsampling_filters.h:129-172", "filters.h:131-169", "mixers.h:169-188"):
        assert cite in doc, cite


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("stream_set_grid_cap", "stream_get_grid_cap", "stream_grid_stats"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name


def _stats(lib):
    v = [C.c_ulong(7) for _ in range(2)]
    assert lib.srcdsp_stream_grid_stats(*[C.byref(x) for x in v]) == 0
    return [x.value for x in v]


def test_stats_skip_null_pointers(capi):
    lib = capi.lib()
    assert lib.srcdsp_stream_grid_stats(None, None) == capi.OK
    a, b = C.c_ulong(7), C.c_ulong(7)
    assert lib.srcdsp_stream_grid_stats(C.byref(a), None) == capi.OK
    assert lib.srcdsp_stream_grid_stats(None, C.byref(b)) == capi.OK
    assert [a.value, b.value] == _stats(lib) == _stats(lib)
    assert b.value <= a.value  # a looping launch is a launch


def test_setter_refuses_a_negative_cap_and_takes_a_cap_and_zero(capi):
    import srcdsp_amd as S
    lib = capi.lib()
    before = _stats(lib)
    assert lib.srcdsp_stream_get_grid_cap() == 0
    assert lib.srcdsp_stream_set_grid_cap(-1) == capi.ERR_ARG
    assert b"stream_set_grid_cap" in lib.srcdsp_last_error()
    assert lib.srcdsp_stream_get_grid_cap() == 0  # a refused call changes nothing
    try:
        assert lib.srcdsp_stream_set_grid_cap(3) == capi.OK
        assert lib.srcdsp_stream_get_grid_cap() == 3 and S.stream_get_grid_cap() == 3
    finally:
        assert lib.srcdsp_stream_set_grid_cap(0) == capi.OK
    assert lib.srcdsp_stream_get_grid_cap() == 0
    with pytest.raises(S.SrcdspError) as e:
        S.stream_set_grid_cap(-5)
    assert e.value.code == capi.ERR_ARG
    S.stream_set_grid_cap(0)
    assert S.stream_get_grid_cap() == 0
    assert list(S.stream_grid_stats()) == _stats(lib) == before  # no launch was made


def test_a_named_older_build_loads_and_the_shipped_one_must_be_whole(capi):
    """A library named by SRCDSP_HIP_LIB (an A/B base build, a test variant
    linked from an older tree) may lack an entry point added since: it loads,
    and only the call it lacks raises.  The shipped library gets no such
    allowance: an entry point of the table it does not export fails the load."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C\n"
            "from srcdsp_amd import _capi as A\n"
            "A.SIGNATURES['srcdsp_not_in_this_build'] = (C.c_int, [])\n"
            "try:\n"
            "    lib = A.lib()\n"
            "except AttributeError as e:\n"
            "    print('load refused', 'srcdsp_not_in_this_build' in str(e))\n"
            "else:\n"
            "    assert lib.srcdsp_stream_set_grid_cap(0) == 0\n"
            "    try:\n"
            "        A.call('srcdsp_not_in_this_build')\n"
            "    except AttributeError as e:\n"
            "        print('call refused', 'srcdsp_not_in_this_build' in str(e))\n")
    env = {k: v for k, v in os.environ.items() if k != "SRCDSP_HIP_LIB"}
    for named, want in ((False, "load refused True"), (True, "call refused True")):
        e = dict(env, SRCDSP_HIP_LIB=capi.LIB_PATH) if named else env
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip().splitlines()[-1] == want, r.stdout
