"""What libccm_host.so exports and what ccm_host_c.h declares, on the CPU: the library's ccmh_* entry points are the names of tests/golden/host_c_symbols.txt
(the list as the single-file mirror exported it), the header declares exactly those, and the calling thread's contexts have one owner: one thread_context
function in the whole library, however many translation units call it.  Reads the built library and the header only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ccm_slam_amd", "libccm_host.so")
HEADER = os.path.join(ROOT, "ccm_slam_amd", "host", "ccm_host_c.h")


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "host_c_symbols.txt")) as f:
        names = f.read().split()
    assert len(names) == len(set(names)) == 150
    return set(names)


def _nm(*flags):
    return [line.split(None, 2) for line in subprocess.check_output(["nm", *flags, LIB], text=True).splitlines()]


def test_exported_c_entry_points_are_the_golden_list():
    exported = {f[2] for f in _nm("-D", "--defined-only") if len(f) == 3 and f[2].startswith("ccmh_")}
    assert exported == _golden(), (sorted(exported - _golden()), sorted(_golden() - exported))


def test_header_declares_every_exported_entry_point_and_nothing_else():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    declared = re.findall(r"\b(ccmh_\w+)\s*\(", text)
    assert len(declared) == len(set(declared)), sorted(n for n in set(declared) if declared.count(n) > 1)
    assert set(declared) == _golden(), (sorted(set(declared) - _golden()), sorted(_golden() - set(declared)))


def test_one_thread_context_function_in_the_library():
    # the full symbol table, local symbols included: a copy per translation unit would show here as several lines
    owners = [f for f in _nm("-C") if len(f) == 3 and f[1] in "tTwW" and re.search(r"\bthread_context\(int\)$", f[2])]
    assert len(owners) == 1, owners
