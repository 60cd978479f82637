"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/ctvae_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ctvae_amd.build import build
    build()
    from ctvae_amd import native
    return native


def test_exports_match_header(lib):
    hdr = open(os.path.join(ROOT, "include", "ctvae_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(ctvae_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == lib.EXPORTS, (set(declared) ^ set(lib.EXPORTS))
    handle = lib.load()
    for name in declared:
        assert hasattr(handle, name), name
    assert handle.ctvae_arch() == b"gfx950"
    assert handle.ctvae_workspace_bytes() >= 64 << 20
    assert b"bad argument" in handle.ctvae_error_string(-22)


def test_ctypes_signatures_match_header_prototypes(lib):
    """Every prototype of include/ctvae_hip.h against the ctypes argtypes of native.py: same number of parameters, and
    pointer / int / float / size_t / long in the same positions (a shifted argument would otherwise only show up as a
    wrong result on the GPU)."""
    import ctypes
    hdr = open(os.path.join(ROOT, "include", "ctvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(ctvae_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", hdr, re.S))
    def kind(param):
        param = " ".join(param.split())
        if "*" in param:
            return "ptr"
        t = param.rsplit(" ", 1)[0] if " " in param else param
        return {"int": "int", "float": "float", "size_t": "size", "long": "long", "double": "double"}[t.replace("const ", "")]
    ck = {ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_size_t: "size", ctypes.c_long: "long",
          ctypes.c_char_p: "ptr"}
    checked = 0
    for name, argtypes in lib.SIGNATURES.items():
        params = [p for p in protos[name].split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), f"{name}: header has {len(params)} parameters, native.py {len(argtypes)}"
        for i, (p_, a) in enumerate(zip(params, argtypes)):
            hk, nk = kind(p_), ck[a]
            if {hk, nk} == {"size", "long"}:          # c_size_t and c_long are the same ctypes class on LP64
                continue
            assert hk == nk, f"{name} parameter {i} ({' '.join(p_.split())}): header {hk}, native.py {nk}"
        checked += 1
    assert checked == len(lib.SIGNATURES) >= 50


# ---- the header parser behind native.SIGNATURES / _RESTYPES / EXPORTS: stated independently of it --------------------------
def _header():
    return open(os.path.join(ROOT, "include", "ctvae_hip.h")).read()


def test_parser_finds_every_prototype_of_the_header():
    from ctvae_amd import native
    names = set(re.findall(r"\b(ctvae_[a-z_0-9]+)\s*\(", _header()))
    protos = native.parse_prototypes(_header())
    assert len(protos) == len(names) and set(protos) == names
    assert protos == native.PROTOTYPES and native.EXPORTS == sorted(names)
    assert set(native.SIGNATURES) | set(native._RESTYPES) == names and not set(native.SIGNATURES) & set(native._RESTYPES)
    for name, (restype, argtypes, has_stream) in protos.items():       # the split call() relies on: it appends the stream
        assert (name in native.SIGNATURES) == (restype is ctypes.c_int and has_stream), name
        if name in native.SIGNATURES:
            assert native.SIGNATURES[name] == argtypes and argtypes[-1] is ctypes.c_void_p
        else:
            assert native._RESTYPES[name] is restype


def test_parser_types_of_six_entries_written_by_hand():
    from ctvae_amd import native
    i, l, f, sz, p, s = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
    P = native.PROTOTYPES
    assert P["ctvae_adam_step"] == (i, [p, p, p, p, p, l, f, p], True)
    assert P["ctvae_conv_forward"] == (i, [i, p, p, p, p, p, i, i, i, i, i, i, i, i, i, i, p, p, i, p, p, p, sz, p], True)
    assert len(P["ctvae_conv_forward"][1]) == 24
    assert P["ctvae_prof_report"] == (sz, [s, sz], False)
    assert P["ctvae_error_string"] == (s, [i], False)
    assert P["ctvae_workspace_bytes"] == (sz, [], False)
    assert P["ctvae_glinear_forward"] == (i, [p, i, i, i, i, p, p, p, p, p, p, p, i, i, p], True)
    assert "ctvae_adam_step" in native.SIGNATURES and native._RESTYPES["ctvae_prof_report"] is sz
    assert native._RESTYPES["ctvae_error_string"] is s and "ctvae_workspace_bytes" not in native.SIGNATURES


@pytest.mark.parametrize("proto", ["int ctvae_x(int a, long long n, void* stream);", "int ctvae_x(uint8_t flag);",
                                   "unsigned ctvae_x(int a);", "int ctvae_x(long long);", "int64_t ctvae_x(void);"])
def test_parser_refuses_a_type_it_does_not_know(proto):
    from ctvae_amd import native
    with pytest.raises(RuntimeError) as e:
        native.parse_prototypes(proto)
    assert proto in str(e.value)                 # the message shows the prototype


def test_parser_takes_multi_line_prototypes_and_inline_comments():
    from ctvae_amd import native
    text = """
    #ifdef __cplusplus
    extern "C" {
    #endif
    #define CTVAE_SOMETHING 3 /* not a prototype: ctvae_ghost(int a); */
    /* ctvae_in_a_comment(float x); is not one either */
    const char* ctvae_name(void); // trailing
    int ctvae_two_lines(const float* const* w, /* host array */ int n,
                        size_t ws_bytes,
                        void* stream);
    void
    ctvae_switch(int on, double t);
    size_t ctvae_query(const char* key, int64_t* out, float);
    #ifdef __cplusplus
    }
    #endif
    """
    i, p, s, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
    assert native.parse_prototypes(text) == {
        "ctvae_name": (s, [], False),
        "ctvae_two_lines": (i, [p, i, sz, p], True),
        "ctvae_switch": (None, [i, ctypes.c_double], False),
        "ctvae_query": (sz, [s, p, ctypes.c_float], False),
    }


# ---- one declaration per launcher ------------------------------------------------------------------------------------------
def _csrc_sources():
    d = os.path.join(ROOT, "ct-vae_amd", "csrc")
    return [(f, open(os.path.join(d, f)).read()) for f in sorted(os.listdir(d)) if f.endswith((".hip", ".inc"))]


# column 0: a return type, a name, a parameter list -- closed by `;` (a prototype) or opening a body (a definition)
_FUNC = r"^(?!static_assert\b|typedef\b|using\b|return\b|#)([A-Za-z_][\w:<>,*&\s]*?[\s*&])([A-Za-z_]\w*)\s*\(([^;{}]*)\)\s*"


def test_no_source_file_declares_a_function_it_does_not_define():
    """Prototypes of host functions live in the headers of csrc/ (convpaths.hpp, ops.hpp, tapgemm.hpp, pair.hpp, ...), which the
    defining file includes too; a .hip or .inc that restates one is a second copy nothing checks.  (__device__ declarations
    are not looked at: device code is not linked across files, such a declaration never leaves its file.)"""
    found, nfiles = [], 0
    for name, src in _csrc_sources():
        nfiles += 1
        for m in re.finditer(_FUNC + r";", src, re.M):
            if "__device__" not in m.group(1):
                found.append(f"{name}:{src[:m.start()].count(chr(10)) + 1} {m.group(2)}")
    assert nfiles >= 40 and not found, found
    # the pattern does see a prototype, one line or several, and leaves calls and definitions alone
    sample = "int f(int a);\nbool g(const ConvGeom& g,\n       size_t n);\nint h(int a) { return f(a); }\n  int k(int);\nfoo(1);\n"
    assert [m.group(2) for m in re.finditer(_FUNC + r";", sample, re.M)] == ["f", "g"]


def test_default_arguments_are_stated_in_the_headers_only():
    ndefs, found = 0, []
    for name, src in _csrc_sources():
        for m in re.finditer(_FUNC + r"\{", src, re.M):
            ndefs += 1
            if re.search(r"(?<![=!<>])=\s*(nullptr|0)\b", m.group(3)):
                found.append(f"{name}:{src[:m.start()].count(chr(10)) + 1} {m.group(2)}")
    assert ndefs >= 300 and not found, found
    d = os.path.join(ROOT, "ct-vae_amd", "csrc")
    hdr = open(os.path.join(d, "convpaths.hpp")).read() + open(os.path.join(d, "ops.hpp")).read()
    for fn, defaults in (("launch_bn_forward", 1), ("launch_bn_finish_forward", 2), ("launch_bn_backward", 2),
                         ("launch_loss_forward", 4), ("launch_mse_backward", 1), ("launch_loss_backward", 1)):
        (params,) = re.findall(r"\b%s\(([^;{}]*)\);" % fn, hdr)
        assert len(re.findall(r"=\s*(?:nullptr|0)\b", params)) == defaults, fn


def test_product_path_has_no_cpu_fallback():
    import torch
    from ctvae_amd import kernels as K
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.to_nhwc(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError):
        K.ConvAct.apply(torch.zeros(1, 4, 4, 32), torch.zeros(32, 32, 1, 1), None, None, K.ConvSpec(K.CONV, 32, 32, 1))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "ct-vae_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "/root/reference" not in src, f
