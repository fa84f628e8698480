"""Host only: where the device helpers of csrc/ live. The wave primitives have
their one definition in csrc/wave.h, the f32 directed roundings in
csrc/order.h, and no free __device__ function is defined twice under one name
and parameter list ("One header per kind of helper"). Plain regexes
over the source text; nothing is compiled."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-als-twotower-recommender_amd", "csrc")


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) > 40
    return {os.path.basename(p): open(p).read() for p in paths}


def _code(text):
    """The text without comments (a comment may name a builtin)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _files_with(word):
    return sorted(name for name, text in _sources().items() if re.search(r"\b" + word + r"\b", _code(text)))


def test_wave_barrier_only_in_wave_h():
    assert _files_with("__builtin_amdgcn_wave_barrier") == ["wave.h"]


def test_permlane_swaps_only_in_wave_h():
    assert _files_with("__builtin_amdgcn_permlane16_swap") == ["wave.h"]
    assert _files_with("__builtin_amdgcn_permlane32_swap") == ["wave.h"]


def test_nextafterf_only_in_order_h():
    assert _files_with("nextafterf") == ["order.h"]


# A free function's head: __device__ at the start of a line (members of a
# struct are indented and belong to their struct's name), then everything up
# to the name before the parameter list.
_HEAD = re.compile(r"^(?:(?:static|inline|__host__)\s+)*__device__\b[^;{}()]*?\b([A-Za-z_]\w*)\s*\(", re.M)


def _params(code, start):
    """(text between the parentheses opening at start, index after them)."""
    depth = 0
    for i in range(start, len(code)):
        depth += {"(": 1, ")": -1}.get(code[i], 0)
        if depth == 0:
            return code[start + 1:i], i + 1
    raise AssertionError("unbalanced parentheses")


def _signature(params):
    """The parameter types: per parameter, without default value and name."""
    out, depth, cur = [], 0, ""
    for ch in params + ",":
        if ch == "," and depth == 0:
            p = re.sub(r"=.*", "", cur, flags=re.S).strip()
            p = re.sub(r"\(&\s*\w+\)", "(&)", p)          # T (&name)[N]
            p = re.sub(r"\b[A-Za-z_]\w*\s*$", "", p) if re.search(r"[\s*&]\w+\s*$", p) else p
            p = re.sub(r"\b(__restrict__|const)\b", "", p)
            out.append(re.sub(r"\s+", "", p))
            cur = ""
        else:
            depth += {"(": 1, "<": 1, "[": 1, ")": -1, ">": -1, "]": -1}.get(ch, 0)
            cur += ch
    return ",".join(p for p in out if p)


def _device_definitions():
    defs = {}
    for name, text in _sources().items():
        code = _code(text)
        for m in _HEAD.finditer(code):
            params, end = _params(code, m.end() - 1)
            if not re.match(r"\s*\{", code[end:]):
                continue  # a declaration (the buffer loads bound by __asm)
            defs.setdefault((m.group(1), _signature(params)), set()).add(name)
    return defs


def test_signature_normalisation():
    assert _signature("const float* __restrict__ a, int n") == "float*,int"
    assert _signature("const double (&arow)[KP], const double* v") == "double(&)[KP],double*"
    assert _signature("KV<T> x") == "KV<T>"
    assert _signature("") == ""


def test_no_device_function_defined_twice():
    defs = _device_definitions()
    assert len(defs) > 100  # the scan sees the helpers at all
    assert ("wave_lds_fence", "") in defs and ("lane_read", "T,int") in defs
    twice = {k: sorted(v) for k, v in defs.items() if len(v) > 1}
    assert not twice, twice
