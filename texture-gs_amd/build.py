"""Build libtexgs.so (hipcc, gfx950 only) in-tree.  Usage: python texture-gs_amd/build.py [--force] [--verbose]

One object per unit of UNITS; a stage is one unit (its kernels, launchers, argument checks and C entry points) plus its
header in include/.  An object is rebuilt when its unit or any header of HEADERS is newer; HEADERS is every *.h under
include/ and csrc/, and build_id() hashes the same list.  preprocess.hip is built with -ffp-contract=off (its
fp32 operation order is part of the bit-exact key/rect/radius contract) and so is points.hip (its squared distance is
compared bit for bit), density.hip (its per-step statistics likewise), optim.hip (the Adam step's arithmetic likewise) and
metrics.hip (its fp64 sums are compared with numpy's), present.hip (its output bytes and floats are compared bit for bit) and
ingest.hip (its fp64 tap tables are compared with Pillow's, its bytes and floats bit for bit) and surface.hip (its fp64 inverse and
dot products are compared with numpy's bit for bit) and lpips.hip (its head's (a - b)^2 must equal (b - a)^2 bit for bit) and
lpips_grad.hip (the gradient of the partner must equal the gradient of the first image of the swapped pair bit for bit) and
params.hip (its row arithmetic is compared with numpy's bit for bit, exp and log included) and
retexture.hip (its fp64 taps and blend and its fp32 mode arithmetic are compared with numpy's bit for bit) and
shcolor.hip (its SH evaluation and view direction are compared with numpy's bit for bit);
the render kernels allow contraction
and use hardware fp32 atomics (-munsafe-fp-atomics).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, os.environ.get("TEXGS_LIB_NAME", "libtexgs.so"))     # TEXGS_LIB_NAME: experiment builds
OBJ = os.path.join(HERE, os.environ.get("TEXGS_OBJ_DIR", "build"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
          "-I" + CSRC, "-Wall"]
UNITS = {
    "preprocess.hip": ["-ffp-contract=off"],
    "binning.hip": [],
    # -fno-slp-vectorize: the SLP vectoriser pairs fp32 ops into v_pk_* (packed fp32); in K6 / K7 the register-pair shuffling
    # (v_mov) that feeds them costs more issue slots than the packing saves and 9-14 VGPRs: K6 289 -> 265 us, K7 820 -> 772 us
    "render.hip": ["-munsafe-fp-atomics", "-ffp-contract=fast", "-fno-slp-vectorize"],
    "loss.hip": [],
    "selftest.hip": [],
    "uvnet.hip": [],
    "uvmap.hip": ["-munsafe-fp-atomics"],
    "points.hip": ["-ffp-contract=off"],      # its squared distance is a bit-exact contract: no fused multiply-add
    "cubetex.hip": ["-munsafe-fp-atomics"],   # the texture gradient's scatter: hardware fp32 atomic adds
    "density.hip": ["-ffp-contract=off"],     # the per-step statistics are a bit-exact contract: x*x + y*y with separate roundings
    "metrics.hip": ["-ffp-contract=off"],     # fp64 sums of exact fp32 products, reproducible against numpy: no fused multiply-add
    "optim.hip": ["-ffp-contract=off"],       # the Adam step's arithmetic is a bit-exact contract: one rounding per operation
    "mlp.hip": [],
    "present.hip": ["-ffp-contract=off"],     # its bytes and floats are a bit-exact contract: one rounding per operation, no fused multiply-add
    "ingest.hip": ["-ffp-contract=off"],      # Pillow's fp64 tap tables and the fp32 decode are a bit-exact contract: one rounding per operation
    "surface.hip": ["-ffp-contract=off"],     # the fp64 inverse and dot products are a bit-exact contract: one rounding per operation
    "lpips.hip": ["-ffp-contract=off"],       # the head's (a - b)^2 must equal (b - a)^2 bit for bit: no fused multiply-add
    "lpips_grad.hip": ["-ffp-contract=off"],  # d img1 of (a, b) must equal d img0 of (b, a) bit for bit: one rounding per operation
    "params.hip": ["-ffp-contract=off"],      # the row arithmetic is a bit-exact contract and a row's bits must not depend on n or its position
    "retexture.hip": ["-ffp-contract=off"],   # the fp64 resize and the fp32 mode arithmetic are a bit-exact contract: one rounding per operation
    "shcolor.hip": ["-ffp-contract=off"],     # the SH evaluation in the reference's operation order is a bit-exact contract: one rounding per operation
    "abi.hip": [],
}
# every header a unit can include; the one list that both the rebuild rule (build) and build_id() read
HEADERS = sorted(os.path.join(d, f) for d in (os.path.join(ROOT, "include"), CSRC) for f in os.listdir(d) if f.endswith(".h"))


def build_id():
    """Identity of what libtexgs.so is built FROM: sha256 over the units of UNITS, HEADERS and the compile flags (16 hex digits).
    build() bakes it into the library (texgs_build_id()); texgs/_lib.py recomputes it from the tree and refuses a library that
    was built from other sources -- the prebuilt .so is what travels to the GPU box, mtimes do not."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.path.join(CSRC, u) for u in UNITS) + HEADERS:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    h.update(repr((COMMON[:4], sorted(UNITS.items()), os.environ.get("TEXGS_EXTRA_FLAGS", ""))).encode())
    return h.hexdigest()[:16]


def _newer(src_list, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    objs = []
    bid = build_id()
    idfile = os.path.join(OBJ, "build_id.txt")
    stale_id = not os.path.exists(idfile) or open(idfile).read().strip() != bid
    for src, flags in UNITS.items():
        sp = os.path.join(CSRC, src)
        op = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(op)
        if src == "abi.hip":        # carries the build id: rebuilt whenever any source or flag changed
            flags = flags + ['-DTEXGS_BUILD_ID="%s"' % bid]
        if force or _newer([sp] + HEADERS + [os.path.abspath(__file__)], op) or (src == "abi.hip" and stale_id):
            cmd = [HIPCC] + COMMON + flags + os.environ.get("TEXGS_EXTRA_FLAGS", "").split() + ["-c", sp, "-o", op]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    if force or _newer(objs, LIB):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with open(idfile, "w") as f:
        f.write(bid + "\n")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv or True))
