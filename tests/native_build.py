"""TEST INFRASTRUCTURE: the one place a native reference under tests/native/ is compiled."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def build(sources, name):
    """sources: a tuple of file names under tests/native/ -> the path of lib<name>.so, built once per process with g++ and the flags of oracle/Makefile
    (the oracle's floating-point contract: -ffp-contract=off, no FMA)"""
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1).split()
    so = os.path.join(tempfile.mkdtemp(prefix=name + "_"), "lib%s.so" % name)
    subprocess.check_call(["g++"] + flags + ["-shared", "-I" + os.path.join(ROOT, "oracle")] + [os.path.join(ROOT, "tests", "native", f) for f in sources] + ["-o", so])
    return so
