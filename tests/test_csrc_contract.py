"""The host/kernel contract of rgbd_pl_slam_amd/csrc is written once: the library is linked from separately compiled *_host.hip and *_kernels.hip files,
so an argument struct, a grid / LDS constant or a kernel signature stated in two files can drift apart without a link error.  Source text only."""
import collections
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rgbd_pl_slam_amd", "csrc")


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(CSRC, name)) as f:
                text = f.read()
            out[name] = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)   # comments may speak of anything
    return out


SRC = _sources()
HIP = {name: text for name, text in SRC.items() if name.endswith(".hip")}


def _defined_twice(pattern, exempt=lambda name, text: False):
    where = collections.defaultdict(set)
    for name, text in SRC.items():
        for m in re.finditer(pattern, text, flags=re.M):
            if not exempt(m.group(1), text):
                where[m.group(1)].add(name)
    return {k: sorted(v) for k, v in where.items() if len(v) > 1}


def test_sources_found():
    assert len(HIP) >= 20 and "plf_common.h" in SRC


def test_every_struct_is_defined_in_one_file():
    assert _defined_twice(r"^[ \t]*struct[ \t]+(\w+)[^;{()]*\{") == {}


def test_every_macro_is_defined_in_one_file():
    # a name its file also #undefs is a local helper (ALLOC of the *_create functions)
    undefd = lambda name, text: re.search(r"^[ \t]*#[ \t]*undef[ \t]+%s\b" % name, text, flags=re.M) is not None
    assert _defined_twice(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", undefd) == {}


def test_no_kernel_is_declared_in_a_hip_file():
    # __global__ up to the first ';' or '{': a definition reaches its body first
    found = {name: re.findall(r"__global__[^;{]*;", text) for name, text in HIP.items()}
    assert {k: v for k, v in found.items() if v} == {}


def test_no_plf_function_is_declared_in_a_hip_file():
    found = {}
    for name, text in HIP.items():
        protos = re.findall(r"^[A-Za-z_][\w \t*&:<>\"]*\bplf_\w+[ \t]*\([^;{}]*\)[ \t]*;", text, flags=re.M)
        protos = [p for p in protos if not re.match(r"static\b|extern[ \t]+\"C\"|return\b|typedef\b", p)]
        if protos:
            found[name] = protos
    assert found == {}
