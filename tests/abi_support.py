"""The recipe of the tests/test_*_abi.py modules, as functions over a feature's data: include/vf_hip.h, cabi.SYMBOLS, the ctypes
prototypes and the exported library agree on a feature's entry points, defines and info struct; the header's comment documents the
calls; NULL handles are refused; the pybind signatures hold on Scene and TerrainSpike of both packages.

Every function that reads the header takes its text as an optional last argument (default: include/vf_hip.h), so that the functions
can themselves be held to a doctored text (tests/test_support.py).  Nothing native is imported when this module is."""
import ctypes
import os
import re

from support import ROOT

HEADER = os.path.join(ROOT, "include", "vf_hip.h")


def header_text(text=None):
    return open(HEADER).read() if text is None else text


def code(text=None):
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", header_text(text), flags=re.S)


def prototypes(names, text=None):
    """{name: [parameter names]} of the header's `int name(...)` declarations"""
    src = code(text)
    out = {}
    for n in names:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), f"{n} is not declared in include/vf_hip.h"
        params = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src).group(1)
        out[n] = [re.sub(r"\[\d*\]", "", a.split()[-1]).lstrip("*") for a in params.split(",")]
    return out


def check_entry_points(spec, text=None):
    """spec: {name: [parameter names]}.  Each name is declared with those parameters, listed in cabi.SYMBOLS with a ctypes prototype of
    as many arguments, and exported by the library."""
    from vulkan_forge_amd import cabi
    got = prototypes(spec, text)
    lib, loaded = ctypes.CDLL(cabi.DEFAULT_LIB), cabi.load()
    for n, params in spec.items():
        assert n in cabi.SYMBOLS and n in cabi._PROTOS, f"{n} is not listed in cabi.SYMBOLS"
        assert hasattr(lib, n), f"libvf_hip.so does not export {n}"
        assert got[n] == list(params), (n, got[n])
        assert len(getattr(loaded, n).argtypes) == len(params), n


def check_defines(prefix, pairs, text=None):
    """#define VF_<prefix>_<K> <v> for every (K, v), the value whole"""
    src = code(text)
    for k, v in pairs:
        assert re.search(rf"#define VF_{prefix}_{k} {re.escape(str(v))}(\s|$)", src), f"VF_{prefix}_{k}"


def struct_fields(c_name, text=None):
    body = re.search(r"typedef struct " + c_name + r" \{(.*?)\} " + c_name + ";", code(text), flags=re.S).group(1)
    return [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]


def check_info_struct(c_name, ctypes_struct, size, text=None):
    """the struct an info call fills: the header's fields are the ctypes.Structure's, in order, and it has the size"""
    fields = struct_fields(c_name, text)
    assert fields == [f for f, _ in ctypes_struct._fields_], (c_name, fields)
    assert ctypes.sizeof(ctypes_struct) == size, (c_name, ctypes.sizeof(ctypes_struct))
    return fields


def check_header_documents(anchor, names, words, text=None, until=None):
    """from the feature's anchor on (up to `until`, if given), the header's comment has a paragraph per call and every phrase"""
    text = header_text(text)
    assert anchor in text, f"the header's comment has no {anchor!r}"
    block = text[text.index(anchor):text.index(until) if until else None]
    for n in names:
        assert re.search(r"\* " + n + r":", block), f"{n} has no paragraph in the header's comment"
    for word in words:
        assert word in block, word
    return block


def check_null_refusals(calls):
    """calls: (name, args after the handle).  Every call refuses a NULL handle, and needs no device to do so."""
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    for name, args in calls:
        assert getattr(lib, name)(None, *args) == cabi.VF_ERR_INVALID, name


def check_method_docs(cls, patterns, cabi_methods=()):
    """patterns: {method: regular expression its pybind signature matches} on `cls` of both packages; cabi_methods: on cabi.Terrain"""
    import vulkan_forge
    import vulkan_forge_amd
    from vulkan_forge_amd import cabi
    for pkg in (vulkan_forge, vulkan_forge_amd):
        T = getattr(pkg, cls)
        for meth, pattern in patterns.items():
            doc = getattr(T, meth).__doc__
            assert re.search(pattern, doc), (pkg.__name__, cls, meth, doc)
    for name in cabi_methods:
        assert callable(getattr(cabi.Terrain, name)), name
