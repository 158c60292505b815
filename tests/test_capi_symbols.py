"""The C-ABI library builds, loads, and exports every symbol include/kvpress_hip.h declares.
No compute is launched (no GPU here): only calls that return before touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from kvpress_amd import build as B

    B.build()
    from kvpress_amd import _native

    return _native.lib()


def declared_symbols(headers=("kvpress_hip.h",)):
    names = set()
    for h in headers:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names |= set(re.findall(r"\b(kvp_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


def test_hot_path_boundary_has_no_out_of_scope_entry_points():
    """include/kvpress_hip.h is SURVEY section 8's boundary and nothing else: the round-1 extras (SURVEY section 2 out of scope) live in
    kvpress_hip_extra.h and their own shared library, measurement / test aids in kvpress_hip_lab.h."""
    main = declared_symbols(("kvpress_hip.h",))
    assert not [n for n in main if any(t in n for t in ("lagkv", "think", "observed", "rowl1", "zero_channels", "prof", "clock_probe", "occupy", "tuning"))]
    assert set(declared_symbols(("kvpress_hip_extra.h",))) >= {"kvp_lagkv_score", "kvp_think_channel_scores", "kvp_observed_attention_score"}
    assert set(declared_symbols(("kvpress_hip_lab.h",))) == {"kvp_prof_enable", "kvp_prof_count", "kvp_prof_get", "kvp_clock_probe", "kvp_occupy_cus",
                                                            "kvp_tuning_reload"}


def test_boundary_entries_cite_the_reference():
    """every entry of the boundary header sits under a comment that names the reference lines it replaces (file.py:line), apart from
    the three pieces of plumbing (version, last error, asynchronous-error poll) and the *_workspace_bytes companions"""
    text = open(os.path.join(ROOT, "include", "kvpress_hip.h")).read()
    plumbing = {"kvp_version", "kvp_last_error", "kvp_async_error_check"}
    last_comment, uncited = "", []
    for m in re.finditer(r"/\*.*?\*/|\b(kvp_[a-z0-9_]+)\s*\(", text, flags=re.S):
        if m.group(0).startswith("/*"):
            if len(m.group(0)) > 120:     # a section comment, not an inline remark
                last_comment = m.group(0)
        elif m.group(1) not in plumbing and not m.group(1).endswith("_workspace_bytes"):
            if not re.search(r"[a-z_]+\.py:\d+", last_comment):
                uncited.append(m.group(1))
    assert not uncited, f"boundary entries without a reference citation: {uncited}"


def test_header_symbols_exported(lib):
    from kvpress_amd import _native

    names = declared_symbols()
    assert len(names) >= 16
    for n in names + declared_symbols(("kvpress_hip_lab.h",)):
        assert hasattr(lib, n), f"{n} declared in include/ but not exported by libkvpress_hip.so"
    clib = _native.contrib_lib()
    for n in declared_symbols(("kvpress_hip_extra.h",)):
        assert hasattr(clib, n), f"{n} declared in include/kvpress_hip_extra.h but not exported by libkvpress_hip_contrib.so"
        assert n not in names


def test_product_library_exports_no_contrib_kernels():
    import subprocess

    from kvpress_amd import _native

    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert "kvp_topk_select" in out
    assert not [l for l in out.splitlines() if any(t in l for t in ("lagkv", "think", "observed_attention", "zero_channels"))]


def _exported(path):
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def internal_api():
    """the C++ functions kvp_host.h marks KVP_INTERNAL_API (what csrc/contrib/*.hip link against in the product library)"""
    text = open(os.path.join(ROOT, "kvpress_amd", "csrc", "kvp_host.h")).read()
    return sorted(set(re.findall(r"^KVP_INTERNAL_API\s[^;(]*?\b(\w+)\s*\(", text, flags=re.M)))


# Kernel handles the toolchain emits (weak, default visibility) for the one kernel template with external linkage, snapkv_p2_asm in
# snapkv_mfma.hip; every other kernel sits in an anonymous namespace.  By exact name.
TOOLCHAIN_SYMBOLS = {"_Z13snapkv_p2_asmILi1EEv8SnapArgsjPKfPfS3_PKj", "_Z13snapkv_p2_asmILi2EEv8SnapArgsjPKfPfS3_PKj"}
# hipcc's one-byte marker per translation unit: the 16 hex digits are a hash over the source PATH and the options, so they differ from
# checkout to checkout and cannot be listed by exact name -- the full form is matched instead, nothing looser
HIP_CUID = re.compile(r"__hip_cuid_[0-9a-f]{1,16}")


def test_libraries_export_only_what_the_headers_declare(lib):
    """the converse of test_header_symbols_exported: the libraries are built with -fvisibility=hidden, so their dynamic symbol tables
    hold the extern "C" entries of their headers, the KVP_INTERNAL_API functions of kvp_host.h (product library only), and nothing else"""
    from kvpress_amd import _native

    internal = internal_api()
    assert internal and all(n.startswith("kvp_") for n in internal)
    for path, headers, allowed_cxx in ((_native.LIB_PATH, ("kvpress_hip.h", "kvpress_hip_lab.h"), internal),
                                       (_native.CONTRIB_LIB_PATH, ("kvpress_hip_extra.h",), [])):
        declared = set(declared_symbols(headers))
        mangled_ok = tuple(f"_Z{len(n)}{n}" for n in allowed_cxx)
        stray = []
        for s in _exported(path):
            if s in declared or s in TOOLCHAIN_SYMBOLS or HIP_CUID.fullmatch(s):
                continue
            if mangled_ok and s.startswith(mangled_ok):   # (the length prefix of the mangling makes this the exact function name)
                continue
            stray.append(s)
        assert not stray, f"{os.path.basename(path)} exports symbols outside its headers: {stray}"


def test_no_hand_written_prototypes_of_other_files_functions():
    """a function that one .hip defines and another calls is declared in a header (kvp_host.h or its family's *_internal.h), never by a
    body-less prototype typed again in the calling .hip"""
    csrc = os.path.join(ROOT, "kvpress_amd", "csrc")
    files = [os.path.join(d, f) for d, _, fs in os.walk(csrc) for f in fs if f.endswith(".hip")]
    assert len(files) >= 20
    # a declarator at column 0: specifiers / return type, name, balanced parameter list, then `;` (prototype) or `{` (definition)
    pat = re.compile(r'^(?![ \t#/}])(?:[\w:<>*&"]+[ \t]+)+[*&]?(\w+)\((?:[^;{}()]|\([^()]*\))*\)\s*(;|\{)', flags=re.M)
    defined, protos = {}, []
    for f in files:
        text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(f).read(), flags=re.S))
        for m in pat.finditer(text):
            if m.group(2) == "{":
                defined.setdefault(m.group(1), set()).add(f)
            else:
                protos.append((f, m.group(1)))
    assert "kvp_rownorm_launch" in defined and "kvp_gather_kv" in defined     # the pattern sees the functions this is about
    bad = [(os.path.basename(f), n) for f, n in protos if defined.get(n, set()) - {f}]
    assert not bad, f"prototypes of functions defined in another .hip (declare them in kvp_host.h): {bad}"


def test_host_plumbing_is_spelled_once():
    """csrc/kvp_host.h holds the one workspace arena (KvpArena) and the one place that raises a kernel's dynamic LDS limit
    (kvp_raise_dynamic_lds): no .hip carves a workspace with a local `take` lambda, and nothing under csrc/ but kvp_host.h names the
    attribute"""
    csrc = os.path.join(ROOT, "kvpress_amd", "csrc")
    files = [os.path.join(d, f) for d, _, fs in os.walk(csrc) for f in fs if f.endswith((".hip", ".h", ".inc"))]
    assert len([f for f in files if f.endswith(".hip")]) >= 20
    raises = sorted(os.path.relpath(f, csrc) for f in files if "hipFuncAttributeMaxDynamicSharedMemorySize" in open(f).read())
    assert raises == ["kvp_host.h"], f"the dynamic LDS limit is raised outside kvp_raise_dynamic_lds: {raises}"
    takes = sorted(os.path.relpath(f, csrc) for f in files if f.endswith(".hip") and re.search(r"\bauto\s+take\s*=\s*\[", open(f).read()))
    assert not takes, f"hand-rolled workspace carvers (use KvpArena): {takes}"


C_TYPES = {"void": None, "char": ctypes.c_char, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


def _c_type(text):
    """a C type as the headers spell it -> (number of `*`, ctypes type of the value / of what is pointed to; None for void).
    An unknown type fails the test instead of being skipped."""
    words = re.sub(r"\bconst\b", " ", text).replace("*", " * ").split()
    depth, base = words.count("*"), [w for w in words if w != "*"]
    if base == ["kvp_stream_t"]:      # typedef void* kvp_stream_t
        depth, base = depth + 1, ["void"]
    assert len(base) == 1 and base[0] in C_TYPES and (depth or base[0] != "void"), f"unknown C type {text!r}"
    return depth, C_TYPES[base[0]]


def declared_prototypes(headers=("kvpress_hip.h",)):
    """{name: (return type, [parameter types])} of every kvp_* prototype, each type as _c_type gives it"""
    protos = {}
    for h in headers:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for ret, name, params in re.findall(r"^([A-Za-z_][\w \t*]*?)\b(kvp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
            params = [p.strip() for p in params.split(",")]
            if params == ["void"]:
                params = []
            # a parameter is `type name`: the name is the last identifier
            protos[name] = (_c_type(ret), [_c_type(re.fullmatch(r"(.*?)\b[A-Za-z_]\w*", p, flags=re.S).group(1)) for p in params])
    return protos


def _binds(ctype, c_type):
    """does the ctypes type of a signature table bind the C type?  Values by exact type; any pointer (kvp_stream_t is one) as c_void_p,
    or as a typed pointer whose pointee matches (c_char_p for `const char*`, POINTER(c_float) for `float*`)."""
    depth, base = c_type
    if depth == 0:
        return ctype is base
    if ctype is ctypes.c_void_p:
        return True
    if ctype is ctypes.c_char_p:
        return (depth, base) == (1, ctypes.c_char)
    pointee = getattr(ctype, "_type_", None)
    return isinstance(pointee, type) and _binds(pointee, (depth - 1, base))


def signature_mismatches(table, protos):
    bad = []
    for name, (res, args) in table.items():
        ret, params = protos[name]
        if not _binds(res, ret):
            bad.append(f"{name}: returns {ret}, bound as {res.__name__}")
        if len(args) != len(params):
            bad.append(f"{name}: {len(params)} parameters, bound with {len(args)}")
        bad += [f"{name}: parameter {i} is {p}, bound as {a.__name__}" for i, (a, p) in enumerate(zip(args, params)) if not _binds(a, p)]
    return bad


def test_binding_covers_header(lib):
    """the three signature tables of the binding against the three headers: the same names, and per entry the return type and the
    arity, order and type of the parameters (a c_int for an int64_t, or a c_float for a double, shifts every later argument)"""
    from kvpress_amd import _native

    assert sorted(_native.SIGNATURES) == declared_symbols()
    assert sorted(_native.LAB_SIGNATURES) == declared_symbols(("kvpress_hip_lab.h",))
    assert sorted(_native.CONTRIB_SIGNATURES) == declared_symbols(("kvpress_hip_extra.h",))
    for table, header in ((_native.SIGNATURES, "kvpress_hip.h"), (_native.LAB_SIGNATURES, "kvpress_hip_lab.h"),
                          (_native.CONTRIB_SIGNATURES, "kvpress_hip_extra.h")):
        protos = declared_prototypes((header,))
        assert sorted(protos) == declared_symbols((header,))     # the prototype scan sees every entry the name scan sees
        bad = signature_mismatches(table, protos)
        assert not bad, f"_native's table disagrees with include/{header}: {bad}"


def test_version_and_errors(lib):
    assert lib.kvp_version() == 100
    # k > S is rejected before any HIP call
    rc = lib.kvp_topk_select(None, 1, 10, 10, 11, 0, None, None, 0, None)
    assert rc == -1 and b"bad shape" in lib.kvp_last_error()
    rc = lib.kvp_topk_select(None, 1, 10, 10, 5, 7, None, None, 0, None)   # no such order
    assert rc == -1 and b"bad order" in lib.kvp_last_error()
    rc = lib.kvp_topk_select(None, 1, 10, 10, 5, 1, None, None, 0, None)   # KVP_ORDER_SCORE: arguments are still checked
    assert rc == -1 and b"null pointer" in lib.kvp_last_error()
    rc = lib.kvp_rownorm_score(None, 7, 1, 1, 1, 1, 1, 1, 1, ctypes.c_float(1.0), None, None)
    assert rc == -1 and b"dtype" in lib.kvp_last_error()
    # snapkv: S must exceed the window (snapkv_press.py:84-86), kernel_size odd
    rc = lib.kvp_snapkv_score(None, 0, 0, 0, None, 0, 0, 0, 2, 1, 4, 2, 64, 64, 128, 5, None, None, 0, None)
    assert rc == -1 and b"greater than the window size" in lib.kvp_last_error()
    rc = lib.kvp_snapkv_score(None, 0, 0, 0, None, 0, 0, 0, 2, 1, 4, 2, 100, 64, 128, 4, None, None, 0, None)
    assert rc == -1 and b"odd" in lib.kvp_last_error()
    # ea: more tokens than n_sink (expected_attention_press.py:137)
    rc = lib.kvp_ea_score(None, 0, 0, 0, None, 0, 0, 0, 2, None, None, 1, 4, 2, 4, 128, 4, 1, ctypes.c_float(0.0), None, None, 0, None)
    assert rc == -1 and b"n_sink" in lib.kvp_last_error()


def test_workspace_sizes(lib):
    # Llama-3.1-8B, 128k: a few MiB of scratch, never anything of size [Hq, W, S]
    assert 0 < lib.kvp_topk_workspace_bytes(8, 131072, 65536) < 2 << 20
    ws = lib.kvp_snapkv_workspace_bytes(1, 32, 8, 131072, 64, 128)
    assert 4 << 20 < ws < 16 << 20
    assert lib.kvp_ea_score_workspace_bytes(1, 32, 8, 131072, 128) < 32 << 20


def test_no_cpu_fallback():
    import torch

    import kvpress_amd as P
    from kvpress_amd._native import KvpressHipError

    k = torch.zeros(1, 2, 16, 8)
    with pytest.raises(KvpressHipError):
        P.KnormPress(0.5).compress(None, None, k, k, None, {})
    # ratio 0 short-circuits before any kernel (scorer_press.py:86-87)
    k0, v0 = P.KnormPress(0.0).compress(None, None, k, k, None, {})
    assert k0 is k and v0 is k
    with pytest.raises(AssertionError):
        P.KnormPress(1.0)


def test_product_never_imports_oracle():
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "kvpress_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                t = open(os.path.join(d, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", t, flags=re.M) or "kvpress_oracle" in t:
                    bad.append(f)
    assert not bad, f"product files reference the oracle: {bad}"


def test_generated_asm_loops_are_up_to_date():
    """kvpress_amd/csrc/snapkv_asm.inc is generated by tools/gen_stage_asm.py: the committed file must be what the generator emits."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_stage_asm", os.path.join(root, "tools", "gen_stage_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("GEN_")}
    try:
        spec.loader.exec_module(gen)
    finally:
        os.environ.update(env)
    assert open(os.path.join(root, "kvpress_amd", "csrc", "snapkv_asm.inc")).read() == gen.gen_kernel_inc()


def test_clock_lab_patch_points_exist():
    """tools/make_clock_lab.py (the in-kernel clock stamps behind profiles/rNN_clock_power.txt) patches snapkv_mfma.hip and gather.hip at
    textual markers; an edit that moves one of them must fail HERE, not in the middle of a GPU run (round 6: a comment did)."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_clock_lab", os.path.join(root, "tools", "make_clock_lab.py"))
    lab = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lab)
    for name, fn in (("snapkv_mfma", lab.patch_snapkv), ("gather", lab.patch_gather)):
        src = open(os.path.join(root, "kvpress_amd", "csrc", name + ".hip")).read()
        out = fn(src)
        assert "kvp_lab_begin(0);" in out and "kvp_lab_end(" in out and len(out) > len(src)
