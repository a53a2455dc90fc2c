"""The C ABI of include/hode.h as data: one prototype per entry-point family, in the header's order and the header's words (types
only; `T xN` stands for N consecutive parameters of type T), and the ctypes marshalling built from it.  A family whose prototype
names `R` is a pair hode_<name>_f32 / _f64 with R = float / double; any other is the one symbol hode_<name>.  bind() sets restype
and argtypes of every symbol when the library is loaded; tests/test_capi_abi_host.py holds this table to the header, prototype by
prototype."""
import ctypes as C
import re

import torch


class HodeError(RuntimeError):
    pass


_IN3 = "const R*, int, const R*, int, const R*, int"                    # meal, tvns, gd, each with its mode
_RHS = "void*, int, const R* x7, int x2"
_TAPED = f"void*, int x2, const R*, int, {_IN3}, const R* x2, int x5, const int32_t* x2"         # a taped solve, up to its tape
_BWD = _TAPED + ", void*, const R*"
_JVP = _TAPED + ", const void*, int, const R* x2, R*"

ABI = {
    "version": "const char*()",
    "nn_param_count": "int(int x2)",
    "tape_bytes_hl": "size_t(int x5)",
    "tape_bytes": "size_t(int x4)",
    "rhs_fwd": f"int({_RHS}, R*)",
    "rhs_bwd": f"int({_RHS}, const R*, R* x4)",
    "solve_fwd": f"int(void*, int x2, const R* x2, int, {_IN3}, const R* x2, int x4, double x2, int, R*, int32_t* x3, void*)",
    "solve_bwd": f"int({_BWD}, R* x3)",
    "solve_bwd_inputs": f"int({_BWD}, R* x6)",
    "solve_jvp": f"int({_JVP})",
    "solve_jvp_any": f"int({_JVP})",
    "rhs_bwd_inputs": f"int({_RHS}, const R*, R* x7)",
    "adam_step_f32": "int(void*, int64_t, float*, const float*, float* x2, float x4, int, float x3, void*)",
    "mse_fwd_bwd_f32": "int(void*, int64_t, const float* x2, float, double*, float*)",
    "selftest_xlane": "int(void*, int32_t*)",
    "4gi_default_params": "int(int, double*)",
    "4gi_generate_f64": "int(void*, int x2, double, int, const double* x2, int, const double* x2, int, const double*, double, int64_t, "
                        "double x2, int, double*, int32_t*)",
    "4gi_rhs_f64": "int(void*, int x2, const double* x4, double*)",
    "4gi_windows_f32": "int(void*, const double*, int x2, double, int x8, const int64_t*, int64_t x2, int, float* x4, double*, void*)",
    "4gi_window_moments_f64": "int(void*, const double*, int x7, const int64_t*, int64_t x2, double*, void*)",
    "mse_sets": "int(void*, int, int64_t, const R* x2, R, double*, R*)",
    "obs_nll_sets": "int(void*, int, int64_t, const R* x2, const uint8_t*, int x2, const double* x4, double* x2, R*)",
    "hmc_refresh": "int(void*, int x3, uint64_t, uint32_t, double, const R*, const double*, const R* x2, const double*, R* x3, double* x3, "
                   "int32_t*)",
    "hmc_leapfrog": "int(void*, int x4, double, const double*, const R*, R* x3, const R* x2, int, const double*, double, const int32_t*, "
                    "int, double* x2, int32_t*, uint32_t, const double* x2, int, R* x2)",
    "hmc_accept": "int(void*, int x4, uint64_t, uint32_t, double, R*, const R*, R*, const R*, double*, const double* x3, const int32_t*, "
                  "double* x2, int32_t*, int, const double* x2, R*, double*, int x2)",
    "hmc_welford": "int(void*, int x4, const R*, double*, R*)",
    "nuts_begin": "int(void*, int x3, const R* x3, const double* x3, R*, double*, int32_t*)",
    "nuts_pre": "int(void*, int x3, uint64_t, uint32_t, const double*, const R*, R*, int32_t*, const int32_t*, uint32_t, const double* x2, "
                "int x2, R* x2)",
    "nuts_post": "int(void*, int x4, uint64_t, uint32_t, const double*, const R*, R* x2, double*, int32_t*, const int32_t*, const R* x2, "
                 "int, const double*, double, const int32_t*, int, uint32_t, const double*, int)",
    "nuts_compact": "int(void*, int, const int32_t*, int32_t* x2)",
    "nuts_finish": "int(void*, int x4, double, R* x2, double*, const R*, const double*, const int32_t*, double* x2, int, const double* x2, "
                   "R*, double*, int x2)",
    "pop_params": "int(void*, int x4, const R*, uint32_t, const double* x3, double, const R*, R*)",
    "pop_grad": "int(void*, int x4, const R* x2, uint32_t, const double* x2, double, R*)",
    "x0_params": "int(void*, int x5, const R*, uint32_t, int, const double* x2, const R*, R*, int, uint32_t, const double* x2, const R*, R*)",
    "x0_grad": "int(void*, int x5, const R*, uint32_t, int, const double* x2, const R*, int, uint32_t, const double*, const R*, R*)",
    "sobol_indices": "int(void*, int x3, const R*, int64_t, int x2, uint64_t, double, double* x7)",
    "pred_fold": "int(void*, int, int64_t, const R* x2, const uint8_t*, const double*, const int32_t*, int64_t, int32_t*, double* x5)",
    "pred_score": "int(void*, int64_t, const int32_t*, const double* x5, const R*, const uint8_t*, const double* x2, int, R* x3, double* x2)",
    "pred_tails": "int(void*, int, int64_t, const R*, const int32_t*, int64_t, int, int32_t*, R* x2)",
    "pred_quantiles": "int(void*, int64_t, int, const int32_t*, R* x2, int, const double*, R*, const R*, const uint8_t*, double* x2)",
    "pred_loo_fold": "int(void*, int, int64_t, const R* x2, const uint8_t*, const double*, const int32_t*, int64_t, int, int32_t*, double* x7)",
    "pred_loo_finish": "int(void*, int64_t, int, double, const int32_t*, const double* x4, double*, const double* x2, R* x5, double* x3)",
    "pf_step": "int(void*, int x2, uint32_t, uint64_t, uint32_t, const R*, const int32_t*, const R*, const uint8_t*, const double* x3, int, "
               "double, double*, R*, int32_t*, double*, int, const R*, R*)",
    "pf_smooth": "int(void*, int x4, uint64_t, uint32_t, const R*, const double*, const R*, const double* x2, int, int32_t*, R*)",
    "pf_params": "int(void*, int x2, uint32_t, uint64_t, uint32_t, const double*, int, R*, const int32_t*, const double* x2, double, double*)",
    "ukf_step": "int(void*, int x3, const int32_t*, double x4, const R*, const int32_t*, const R* x2, const uint8_t*, const double* x4, "
                "int32_t*, double* x2, R* x2, double*)",
}

# The extension headers: entry points that libhode.so exports beside those of include/hode.h, declared in a header of their own
# that includes hode.h.  {header under include/: a table as above}; tests/test_ukf_smooth_host.py and tests/test_ukf_em_host.py
# hold each to its header.
EXTENSIONS = {
    "hode_ukf_smooth.h": {
        "ukf_smooth": "int(void*, int x3, const int32_t*, double x4, const R* x3, const double* x2, const int32_t*, const double* x3, double* x6)",
    },
    "hode_ukf_em.h": {
        "ukf_em_points": "int(void*, int x3, const int32_t*, double, const double* x2, const int32_t*, const R*, R* x2, double*)",
        "ukf_em_stats": "int(void*, int x3, const int32_t*, double x4, const R*, const int32_t*, const double* x4, const int32_t*, const R*, "
                        "const uint8_t*, const double*, double*, int32_t*, double*, int32_t*)",
        "ukf_em_mstep": "int(void*, int x3, const int32_t* x2, const double* x2, const int32_t*, const double*, const int32_t*, const double*, "
                        "double* x4)",
    },
}

# the vocabulary of the header: anything else in a prototype is an error
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float,
           "double": C.c_double}
POINTERS = {"void*": None, "const void*": None, "float*": torch.float32, "const float*": torch.float32, "double*": torch.float64,
            "const double*": torch.float64, "int32_t*": torch.int32, "const int32_t*": torch.int32, "const uint8_t*": torch.uint8,
            "const int64_t*": torch.int64}
_REALS = (("_f32", "float", torch.float32), ("_f64", "double", torch.float64))


class Pointer:
    """The argtypes entry of one pointer parameter.  None is NULL; a tensor gives its data_ptr() and must hold the header's element
    type (void* takes any); a ctypes array, pointer or c_void_p and a plain int address pass as they are."""

    def __init__(self, where, word):
        self.word, self.dtype = word, POINTERS[word]
        dtype, any_dtype, address, Tensor = self.dtype, self.dtype is None, C.c_void_p.from_param, torch.Tensor

        def from_param(v):          # a closure, not a method: this sits on the samplers' launch path, a dozen times per launch
            if type(v) is Tensor and (v.dtype is dtype or any_dtype):
                return address(v.data_ptr())
            if v is None or isinstance(v, (C.Array, C._Pointer, C.c_void_p)):
                return v
            if type(v) is int:
                return address(v)
            if not isinstance(v, Tensor):
                raise TypeError(f"{where} is `{word}`: expected None, a tensor, a ctypes array or pointer or an address, got {type(v).__name__}")
            if not any_dtype and v.dtype != dtype:                    # (a tensor subclass comes this way too)
                raise HodeError(f"{where} is `{word}`, got a {v.dtype} tensor")
            return address(v.data_ptr())
        self.from_param = from_param


def expand(abi=ABI):
    """[(symbol, family, dtype or None, return type, [parameter types])], R and xN resolved: what the table says the header declares."""
    out = []
    for name, proto in abi.items():
        ret, _, params = proto[:-1].partition("(")
        pair = re.search(r"\bR\b", params) is not None
        for sfx, real, dtype in (_REALS if pair else (("", "", None),)):
            words = []
            for w in (params.split(",") if params else ()):
                word, _, times = w.strip().partition(" x")
                words += [re.sub(r"\bR\b", real, word)] * int(times or 1)
            out.append((f"hode_{name}{sfx}", name, dtype, ret, words))
    return out


def ctypes_of(symbol, ret, words):
    """(restype, argtypes) of one expanded prototype; HodeError for a word outside the vocabulary."""
    if ret not in RETURNS:
        raise HodeError(f"{symbol}: return type `{ret}` is outside the vocabulary of the C ABI")
    args = []
    for i, w in enumerate(words, 1):
        if w in SCALARS:
            args.append(SCALARS[w])
        elif w in POINTERS:
            args.append(Pointer(f"{symbol} parameter {i}", w))
        else:
            raise HodeError(f"{symbol}: parameter {i} has type `{w}`, outside the vocabulary of the C ABI")
    return RETURNS[ret], args


SIGNATURES = {sym: (name, dtype) + ctypes_of(sym, ret, words) for sym, name, dtype, ret, words in expand()}
SYMBOLS = list(SIGNATURES)                                            # every symbol include/hode.h declares
EXT_SIGNATURES = {hdr: {sym: (name, dtype) + ctypes_of(sym, ret, words) for sym, name, dtype, ret, words in expand(table)}
                  for hdr, table in EXTENSIONS.items()}
EXT_SYMBOLS = {hdr: list(sigs) for hdr, sigs in EXT_SIGNATURES.items()}   # every symbol each extension header declares


def bind(lib, path):
    """Declare every symbol of the table and of the extension tables on a loaded library.  Returns {(family, dtype or None): function}."""
    fns = {}
    for hdr, sigs in [("hode.h", SIGNATURES)] + list(EXT_SIGNATURES.items()):
        for sym, (name, dtype, restype, argtypes) in sigs.items():
            if not hasattr(lib, sym):
                raise HodeError(f"{path} does not export {sym}, which include/{hdr} declares")
            fn = fns[name, dtype] = getattr(lib, sym)
            fn.restype, fn.argtypes = restype, argtypes
    return fns
