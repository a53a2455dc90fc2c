"""Host-side tests of the typed binding (hode/_abi.py): the signature table against include/hode.h prototype by prototype, the
declarations load() leaves on the library, the pointer parameter class, and real calls through the declared functions that return
before any launch.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

import hode
from hode import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ------------------------------------------------------------------ header = table
def parse_header(text):
    """{symbol: (return type, [parameter types])} of every prototype of a header, in the table's spelling (`const float*`: no
    parameter names, the star on the type).  A type outside the vocabulary of the C ABI raises HodeError: nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M).replace('extern "C" {', " ")
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?[\s\*]+)(hode_\w+)\s*\(([^)]*)\)\s*;", text):
        words = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*((?:const\s+)?\w+)\s*(\**)\s*\w+\s*", p)
            words.append(" ".join(m.group(1).split()) + m.group(2) if m else " ".join(p.split()))   # no match: reported as it stands
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        _abi.ctypes_of(name, ret, words)
        out[name] = (ret, words)
    return out


def test_table_states_the_header():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = parse_header(hdr)
    assert len(declared) == 79 and set(declared) == set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    table = {sym: (ret, words) for sym, _, _, ret, words in _abi.expand()}
    assert list(table) == list(declared)                            # the same names in the header's order
    for sym, sig in declared.items():
        assert table[sym] == sig, sym
    assert hode.capi.SYMBOLS == list(declared)


@pytest.mark.parametrize("proto", ["int hode_new_thing(void *stream, long n);", "int hode_new_thing(void *stream, uint8_t *mask);",
                                   "int hode_new_thing(void *stream, const float **rows);", "float hode_new_thing(void *stream);",
                                   "int hode_new_thing(void *stream, unsigned n);"])
def test_a_type_outside_the_vocabulary_is_reported(proto):
    good = "/* a comment; with(a paren) */\nint hode_fine_f32(void *stream, const float *x, int64_t n);\n"
    assert parse_header(good) == {"hode_fine_f32": ("int", ["void*", "const float*", "int64_t"])}
    with pytest.raises(hode.HodeError, match="hode_new_thing.*outside the vocabulary"):
        parse_header(good + proto)
    with pytest.raises(hode.HodeError, match="outside the vocabulary"):          # the table goes through the same check
        [_abi.ctypes_of(sym, ret, words) for sym, _, _, ret, words in _abi.expand({"bad": "int(void*, long)"})]


# ------------------------------------------------------------------ table = library
def test_load_declares_every_symbol():
    lib = hode.load()
    declared = parse_header(open(os.path.join(ROOT, "include", "hode.h")).read())
    for sym, (ret, words) in declared.items():
        fn = getattr(lib, sym)
        assert fn.restype is _abi.RETURNS[ret], sym
        assert len(fn.argtypes) == len(words), sym
        for at, w in zip(fn.argtypes, words):
            if w in _abi.SCALARS:
                assert at is _abi.SCALARS[w], (sym, w)
            else:
                assert isinstance(at, _abi.Pointer) and at.word == w and at.dtype == _abi.POINTERS[w], (sym, w)


def test_a_library_that_lacks_a_symbol_is_refused_by_name():
    with pytest.raises(hode.HodeError, match="hode_version"):
        _abi.bind(C.CDLL(None), "the C library")


# ------------------------------------------------------------------ the pointer class
def _echo(word):
    """A C function that returns the address it is handed, declared with a Pointer parameter: what reaches the callee."""
    cb = C.CFUNCTYPE(C.c_size_t, C.c_void_p)(lambda p: p or 0)
    fn = C.CFUNCTYPE(C.c_size_t, C.c_void_p)(C.cast(cb, C.c_void_p).value)
    fn.argtypes = [_abi.Pointer("hode_echo parameter 1", word)]
    fn.keep = cb
    return fn


def test_pointer_parameter_conversions():
    echo = _echo("const double*")
    assert echo(None) == 0
    t = torch.arange(4, dtype=torch.float64)
    assert echo(t) == t.data_ptr() and echo(t[1:]) == t.data_ptr() + 8
    arr = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert echo(arr) == C.addressof(arr)
    assert echo(C.c_void_p(16 * 5)) == 80 and echo(C.c_void_p(0)) == 0
    assert echo(C.cast(arr, C.POINTER(C.c_double))) == C.addressof(arr)
    assert echo(0x7f12_3456_7890) == 0x7f12_3456_7890                # a plain address, all 64 bits of it


@pytest.mark.parametrize("word,dtype", [("const float*", torch.float64), ("float*", torch.float64), ("double*", torch.float32),
                                        ("const double*", torch.float32), ("int32_t*", torch.int64), ("const int32_t*", torch.int64),
                                        ("const uint8_t*", torch.bool), ("const int64_t*", torch.int32)])
def test_pointer_parameter_refuses_another_element_type(word, dtype):
    p = _abi.Pointer("hode_some_f32 parameter 4", word)
    with pytest.raises(hode.HodeError, match=r"hode_some_f32 parameter 4 is `" + re.escape(word) + "`, got a " + re.escape(str(dtype))):
        p.from_param(torch.zeros(3, dtype=dtype))
    echo, good = _echo(word), torch.zeros(3, dtype=_abi.POINTERS[word])
    assert echo(good) == good.data_ptr()
    with pytest.raises(C.ArgumentError, match="HodeError"):          # and ctypes stops the call
        echo(torch.zeros(3, dtype=dtype))
    with pytest.raises(C.ArgumentError, match="HodeError"):          # a tensor subclass is held to the same rule
        echo(torch.nn.Parameter(torch.zeros(3, dtype=dtype), requires_grad=False))


def test_void_pointer_takes_any_element_type():
    for word in ("void*", "const void*"):
        echo = _echo(word)
        for dtype in (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool, torch.float16):
            t = torch.zeros(3, dtype=dtype)
            assert echo(t) == t.data_ptr()


@pytest.mark.parametrize("bad", [1.5, "0x10", b"abc", [1, 2], True, C.c_int(3), C.c_double(1.0)])
def test_pointer_parameter_refuses_what_is_no_pointer(bad):
    for word in ("void*", "const double*"):
        with pytest.raises(TypeError, match="hode_some parameter 2"):
            _abi.Pointer("hode_some parameter 2", word).from_param(bad)


def test_wrapper_reports_a_wrong_element_type_as_hode_error():
    """Through hode.capi the refusal is a HodeError that names the function, the parameter and both types (ctypes alone would say
    ArgumentError); nothing was called: the stream is fetched first, and a CPU tensor never gets that far."""
    orig = hode.capi._stream
    hode.capi._stream = lambda: 0
    try:
        st = torch.zeros(4, dtype=torch.int64)
        with pytest.raises(hode.HodeError, match=r"hode_nuts_compact parameter 3 is `const int32_t\*`, got a torch.int64"):
            hode.capi.nuts_compact(4, st, st, st)
        with pytest.raises(TypeError, match="hode_nuts_compact parameter 4"):
            hode.capi.nuts_compact(4, None, 2.5, None)
        with pytest.raises(hode.HodeError, match="unsupported dtype torch.float16"):
            hode.capi.hmc_welford(0, 0, 0, 0, None, None, torch.zeros(1, dtype=torch.float16))
    finally:
        hode.capi._stream = orig


# ------------------------------------------------------------------ real calls that return before any launch
def test_host_entry_points_through_the_declared_functions():
    lib = hode.load()
    for ptype, name, first in ((0, "T2DM", [1.72, 0.0256, 26.5, 9.33]), (1, "HV", [5.36, 0.072])):   # data/generate4GI.py:15-64
        buf = (C.c_double * 26)()
        assert lib.hode_4gi_default_params(ptype, buf) == 0
        assert list(buf) == hode.capi.fourgi_default_params(name) and list(buf)[:len(first)] == first
        assert len(set(buf)) > 20 and all(v > 0 for v in buf)
    assert lib.hode_4gi_default_params(2, (C.c_double * 26)()) == EINVAL
    assert lib.hode_nn_param_count(64, 4) == hode.capi.n_params(64, 4) == 13510
    for B, steps, elem, H, L in ((4096, 300, 4, 64, 4), (64, 300, 8, 128, 5), (3, 77, 4, 32, 2)):
        assert lib.hode_tape_bytes_hl(B, steps, elem, H, L) == hode.capi.tape_nbytes(B, steps, elem, L, H) > 0
    assert lib.hode_tape_bytes_hl(1 << 20, 300, 8, 64, 4) > 1 << 32                # size_t, not int
    assert lib.hode_version().decode() == hode.version()


def _dummies(n):
    """n distinct non-null addresses that are never dereferenced."""
    return [C.c_void_p(16 * (k + 1)) for k in range(n)]


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_chain_entry_points_reject_zero_chains_before_any_launch(sfx):
    """chains_ok refuses C = 0 first; every scalar slot holds a value of its own, so a wrong argtypes length or kind would be a ctypes
    error here, not luck."""
    lib = hode.load()
    p = _dummies(20)
    leapfrog = getattr(lib, f"hode_hmc_leapfrog_{sfx}")
    args = [None, 0, 8, 12, 2, 0.25, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 13510, p[7], 0.75, p[8], 3, p[9], p[10], p[11],
            0x80000001, p[12], p[13], 1, p[14], p[15]]
    assert len(args) == len(leapfrog.argtypes) and leapfrog(*args) == EINVAL
    with pytest.raises(C.ArgumentError):
        leapfrog(*args[:5], p[0], *args[6:])                         # a pointer where the header has `double kick`
    with pytest.raises(C.ArgumentError):
        leapfrog(*args[:13], 13510.5, *args[14:])                    # a float where the header has `int P`
    with pytest.raises(TypeError):
        leapfrog(*args[:-1])                                         # one argument short
    post = getattr(lib, f"hode_nuts_post_{sfx}")
    args = [None, 0, 8, 12, 10, 0xFEDCBA9876543210, 0xFFFFFFF1, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], 13510, p[9], 0.75,
            p[10], 3, 0x80000001, p[11], 1]
    assert len(args) == len(post.argtypes) and post(*args) == EINVAL
    accept = getattr(lib, f"hode_hmc_accept_{sfx}")
    args = [None, 0, 8, 12, 1, 0xFEDCBA9876543210, 0xFFFFFFF1, 0.8, *p[:12], 5, p[12], p[13], p[14], p[15], 7, 3]
    assert len(args) == len(accept.argtypes) and accept(*args) == EINVAL


@pytest.mark.parametrize("sfx,real", [("f32", C.c_float), ("f64", C.c_double)])
def test_mse_sets_with_no_set_is_ok_without_a_launch(sfx, real):
    mse = getattr(hode.load(), f"hode_mse_sets_{sfx}")
    p = _dummies(4)
    assert mse(None, 0, 1 << 40, p[0], p[1], 0.5, p[2], p[3]) == 0                 # int64_t len, plain values
    assert mse(None, 0, C.c_int64(1 << 40), p[0], p[1], real(0.5), p[2], p[3]) == 0
    assert mse(None, -1, 8, p[0], p[1], 0.5, p[2], p[3]) == EINVAL
    with pytest.raises(C.ArgumentError):
        mse(None, 0, C.c_int(8), p[0], p[1], 0.5, p[2], p[3])                      # the header says int64_t
