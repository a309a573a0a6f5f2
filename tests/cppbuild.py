"""The one g++ line that builds a C++ driver of tests/cpp/ against include/plf.hpp, the mock headers of tests/mock/ and the built library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rgbd_pl_slam_amd", "libplf_hip.so")


def build_driver(name, tmp_path, *flags):
    """tests/cpp/NAME.cpp -> tmp_path/NAME, with the caller's warning, optimisation and link flags; returns the program's path"""
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", *flags, "-DPLF_WITH_OPENCV", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "mock"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe), LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib"])
    return exe
