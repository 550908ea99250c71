"""What tools/check_{bgsub,seg,pose}_px.py share: the host build of a csrc/*_px.h header behind a few C loops, and the ctypes pointer of a
numpy array."""
import ctypes
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "autoposeestimation_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I", INC]          # -ffp-contract=off as csrc/Makefile


def compile_src(src, out_name, flags):
    """g++ of the C++ text `src` with FLAGS + flags in a fresh directory -> the path of the output"""
    d = tempfile.mkdtemp(prefix="px_host_")
    with open(os.path.join(d, "px.cpp"), "w") as f:
        f.write(src)
    out = os.path.join(d, out_name)
    subprocess.check_call(["g++"] + FLAGS + list(flags) + [os.path.join(d, "px.cpp"), "-o", out])
    return out


def build(src):
    """the loops of `src` as a shared library"""
    return ctypes.CDLL(compile_src(src, "libpx.so", ["-O2", "-shared", "-fPIC"]))


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)
