"""The one g++ line that builds a C++ driver of tests/cpp/ against include/plf.hpp, the mock headers of tests/mock/ and the built library."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rgbd_pl_slam_amd", "libplf_hip.so")


def hex32(a):
    """the floats of `a` (a number or an array) as the hex of their bits, blank-separated: what rdf() of tests/cpp/scenario_io.h reads"""
    return " ".join("%x" % v for v in np.ascontiguousarray(a, np.float32).view(np.uint32).ravel())


def hex64(values):
    """the same for doubles: what rdd() reads"""
    return " ".join("%x" % struct.unpack("<Q", struct.pack("<d", v))[0] for v in values)


def build_driver(name, tmp_path, *flags):
    """tests/cpp/NAME.cpp -> tmp_path/NAME, with the caller's warning, optimisation and link flags; returns the program's path"""
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", *flags, "-DPLF_WITH_OPENCV", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "mock"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe), LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib"])
    return exe
