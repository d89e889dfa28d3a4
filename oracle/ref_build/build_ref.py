"""Builds oracle/_ref/ref_driver: the reference's DSP classes, compiled unmodified and in place from the reference
tree, against the stand-in headers next to this file, linked with ref_driver.cpp.

Nothing of the reference is copied: its sources are named on the compiler's command line where they lie, and every
object and the binary go to oracle/_ref/, which git ignores.  Without a reference tree (a clean checkout elsewhere,
the GPU machine) build_ref() does nothing and the reference pins fall back to the recorded fixtures.

Flags: -O2 -ffp-contract=off, no -march, no fast-math -- the results must not depend on the box.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
STANDINS = os.path.join(HERE, "standins")
OUT = os.path.join(os.path.dirname(HERE), "_ref")
BINARY = os.path.join(OUT, "ref_driver")
DEFAULT_REFERENCE = "/root/reference"
ENV = "PEBBLE_REFERENCE_DIR"

PEBBLELIB = ["cpx", "mixer", "decimator", "downconvert", "fastfir", "fft", "fftaccelerate", "fftooura", "fftcute", "windowfunction", "fir",
             "iir", "fractresampler", "delayline", "perform", "db", "goertzel", "firfilter", "movingavgfilter", "sampleclock", "fldigifilters"]
APPLICATION = ["processstep", "agc", "noiseblanker", "noisefilter", "dcremoval", "iqbalance", "signalstrength"]
DEMOD = ["demod_am", "demod_sam", "demod_nfm", "demod_wfm", "rdsdecode"]  # rdsdecode only because Demod has a CRdsDecode member
# the Morse modem and the Morse sender: the decoder and the keyer proper, without the plugin shells that bring the GUI
PLUGINS = [("MorseDigitalModem", "morse"), ("MorseDigitalModem", "morsecode"), ("MorseGenDevice", "morsegen")]
FLAGS = ["-std=c++14", "-O2", "-ffp-contract=off", "-DPEBBLELIB_LIBRARY", "-DUSE_FFTACCELERATE", "-w"]


def reference_dir():
    d = os.environ.get(ENV, DEFAULT_REFERENCE)
    return d if os.path.isfile(os.path.join(d, "pebblelib", "decimator.cpp")) else None


def _recipe_files():
    out = [os.path.abspath(__file__), os.path.join(HERE, "ref_driver.cpp")]
    for root, _, files in os.walk(STANDINS):
        out += [os.path.join(root, f) for f in files]
    return out


def _compilers(name):
    # g++ 11 rejects non-ASCII dashes inside a disabled block of db.cpp; clang++ accepts them
    cands = ["g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    if name == "db":
        cands = cands[1:] + cands[:1]
    return [c for c in cands if shutil.which(c)]


def _compile(job):
    name, src, obj, inc = job
    err = None
    for cxx in _compilers(name):
        p = subprocess.run([cxx] + FLAGS + inc + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode == 0:
            return
        err = "%s %s:\n%s" % (cxx, src, p.stdout[-2000:])
    raise RuntimeError("reference build failed: %s" % err)


def build_ref(force=False):
    """-> path of the binary, or None where there is neither a reference tree nor a binary built earlier."""
    ref = reference_dir()
    if ref is None:
        return BINARY if os.path.exists(BINARY) else None
    if (not force) and os.path.exists(BINARY) and all(os.path.getmtime(BINARY) >= os.path.getmtime(f) for f in _recipe_files()):
        return BINARY
    obj_dir = os.path.join(OUT, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    # forward/ holds the stand-ins named like a directory of standins/ ("QtCore") and comes first, so that the name finds the file;
    # the third path lies one level below the directory that holds fftw-3.3.4/, as the reference's fftw.h looks it up
    inc = ["-I" + os.path.join(STANDINS, "forward"), "-I" + STANDINS, "-I" + os.path.join(STANDINS, "QtCore"), "-I" + os.path.join(ref, "pebblelib"),
           "-I" + os.path.join(ref, "application"), "-I" + os.path.join(ref, "application", "demod"),
           "-I" + os.path.join(ref, "plugins", "MorseDigitalModem"), "-I" + os.path.join(ref, "plugins", "MorseGenDevice")]
    jobs = [(n, os.path.join(ref, "pebblelib", n + ".cpp"), os.path.join(obj_dir, n + ".o"), inc) for n in PEBBLELIB]
    jobs += [(n, os.path.join(ref, "application", n + ".cpp"), os.path.join(obj_dir, n + ".o"), inc) for n in APPLICATION]
    jobs += [(n, os.path.join(ref, "application", "demod", n + ".cpp"), os.path.join(obj_dir, n + ".o"), inc) for n in DEMOD]
    jobs += [(n, os.path.join(ref, "plugins", d, n + ".cpp"), os.path.join(obj_dir, n + ".o"), inc) for d, n in PLUGINS]
    jobs += [("Accelerate", os.path.join(STANDINS, "Accelerate", "Accelerate.cpp"), os.path.join(obj_dir, "Accelerate.o"), inc),
             ("ref_driver", os.path.join(HERE, "ref_driver.cpp"), os.path.join(obj_dir, "ref_driver.o"), inc)]
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(_compile, jobs))
    tmp = BINARY + ".tmp"
    subprocess.check_call(["g++", "-o", tmp] + [j[2] for j in jobs] + ["-lm"])
    os.replace(tmp, BINARY)
    return BINARY


if __name__ == "__main__":
    import sys
    print(build_ref(force="--force" in sys.argv))
