"""The whole drop-in surface of the C++ shim (msdfgen_amd/shim/msdfgen_shim.cpp), overload by overload and section geometry by section geometry.

tests/shim/shim_surface.cpp is a client of msdfgen's public headers that calls every function the shim defines in namespace msdfgen with its own argument
form, on contiguous, padded, bottom-up, atlas-interior and differently oriented BitmapSections, and dumps the whole backing buffer of every case.
oracle/Makefile builds it twice: oracle/_ref/shim_surface_hip against the shim (the HIP path) and oracle/_ref/shim_surface_cpu against msdfgen's own
objects with uncached distance queries (the build the suite pins bit for bit against the oracle and the device). The two dumps must be the same bytes.
Both binaries travel with oracle/_ref/; the tests are skipped where they do not exist.

Host-only tests keep the table honest: every msdfgen:: function the shim exports is called, case ids are unique, and the CPU twin's bytes are the
oracle's for one case of every family."""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_npz
from test_gpu_cli import BLOBS, TEARDROP

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(os.path.dirname(HERE), "oracle", "_ref")
HIP, CPU, SHIM = (os.path.join(REF_DIR, n) for n in ("shim_surface_hip", "shim_surface_cpu", "libmsdfgen_hip_shim.so"))


def parse(blob):
    """The records of a dump: ({id: (signature, bytes)} in file order, {meta name: float64 array}); ids as a list too, to see duplicates."""
    cases, metas, ids, at = {}, {}, [], 0
    while at < len(blob):
        end = blob.index(b"\n", at)
        head = blob[at:end].decode().split("\t")
        n = int(head[-1])
        body = blob[end+1:end+1+n]
        assert len(body) == n, head
        if head[0] == "META":
            metas[head[1]] = np.frombuffer(body, np.float64)
        else:
            assert head[0] == "CASE" and len(head) == 4, head
            ids.append(head[1])
            cases[head[1]] = (head[2], body)
        at = end+1+n
    return cases, metas, ids


def run_twin(binary, directory):
    texts = {"a": str(load_npz("shape_a.npz")["desc"]), "blobs": BLOBS, "teardrop": TEARDROP}
    paths = []
    for name, text in texts.items():
        paths.append(os.path.join(str(directory), name+".txt"))
        with open(paths[-1], "w") as f:
            f.write(text)
    out = os.path.join(str(directory), os.path.basename(binary)+".bin")
    r = subprocess.run([binary]+paths+[out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    with open(out, "rb") as f:
        return parse(f.read())


@pytest.fixture(scope="module")
def cpu_twin(tmp_path_factory):
    if not os.path.exists(CPU):
        pytest.skip("oracle/_ref/shim_surface_cpu not built (needs the msdfgen sources)")
    return run_twin(CPU, tmp_path_factory.mktemp("surface_cpu"))


def test_every_exported_overload_is_called_and_ids_are_unique(cpu_twin):
    """nm on the shim: every msdfgen:: function it exports is among the signatures the client reports as called (the msdfgen_hip::*Batch entries and
    the extern "C" helpers have tests/test_gpu_shim.py). A function added to the shim without a case here fails this test."""
    if not os.path.exists(SHIM):
        pytest.skip("oracle/_ref/libmsdfgen_hip_shim.so not built (needs the msdfgen headers)")
    cases, _, ids = cpu_twin
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)
    r = subprocess.run(["nm", "-D", "--defined-only", "-C", SHIM], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = set()
    for line in r.stdout.splitlines():
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1] in "TW" and parts[2].startswith("msdfgen::"):
            exported.add(parts[2].strip())
    called = {sig for sig, _ in cases.values()}
    assert len(exported) >= 50, sorted(exported)
    assert not exported-called, "exported by the shim, never called: %s" % sorted(exported-called)
    assert not called-exported, "called, not exported by the shim: %s" % sorted(called-exported)


# ---- the CPU twin against the oracle, one case per family ----------------------------------------------------------------------------------

def _disturb(px, zero):
    """shim_surface.cpp's disturb(): every third texel mirrored about zero, medians exactly == zero at the corners and along a diagonal."""
    px = px.copy()
    h, w, n = px.shape
    z = np.float32(zero)
    for y in range(h):
        for x in range(w):
            if (x+2*y) % 3 == 0:
                px[y, x] = (z+z)-px[y, x]
            if ((x in (0, w-1)) and (y in (0, h-1))) or (x == y and x % 4 == 1):
                for c in range(min(n, 3)):
                    if not (n >= 3 and c == (x+y) % 3):
                        px[y, x, c] = z
    return px


def test_cpu_twin_equals_the_oracle(cpu_twin, oracle, ref):
    """Ties the twin to the oracle the rest of the suite compares the device with: generate (legacy form, stencil), msdfErrorCorrection, a shapeless
    pass, distanceSignCorrection about .25, rasterize, renderSDF and simulate8bit -- the contiguous cases, whose dump is the packed bitmap."""
    cases, metas, _ = cpu_twin
    w, h = 40, 32

    def shape(name, text):
        hd = ref.shape_from_desc(text)
        ref.prepare(hd)
        s = ref.flatten(hd)
        ref.free(hd)
        return s, metas["frame/%s/%dx%d" % (name, w, h)]
    a, fa = shape("a", str(load_npz("shape_a.npz")["desc"]))
    blobs, fb = shape("blobs", BLOBS)

    def xf(frame, lo, hi):
        return np.array([frame[0], frame[1], frame[2], frame[3], lo/frame[0], hi/frame[0]])

    def same(case, *arrays):
        want = b"".join(np.ascontiguousarray(x).tobytes() for x in arrays)
        got = cases[case][1]
        assert len(got) == len(want), (case, len(got), len(want))
        n = int((np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8)).sum())
        assert n == 0, "%s [%s]: %d bytes differ from the oracle" % (case, cases[case][0], n)

    st = np.zeros((h, w), np.uint8)
    f = oracle.generate(blobs, 3, w, h, xf(fb, -1.5, 1), overlap=False, ec_mode=3, ec_dist=2, min_dev=1.5, min_imp=1.3, stencil=st)
    same("generateMSDF/legacy/blobs/40x32", f, st)
    pre3 = oracle.generate(a, 3, w, h, xf(fa, -1, 1), ec_mode=0)
    st = np.zeros((h, w), np.uint8)
    same("msdfErrorCorrection3/transformation/a/40x32", oracle.error_correction(a, pre3, xf(fa, -1, 1), ec_mode=2, ec_dist=1, min_dev=1.5, min_imp=1.3, stencil=st), st)
    same("msdfFastEdgeErrorCorrection3/transformation/a/40x32", oracle.error_correction(a, pre3, xf(fa, -1, 1), ec_mode=3, ec_dist=0, min_dev=1.5))
    pre4 = oracle.generate(a, 4, w, h, xf(fa, -1, 1), ec_mode=0)
    same("msdfFastDistanceErrorCorrection4/transformation/a/40x32", oracle.error_correction(a, pre4, xf(fa, -1, 1), ec_mode=1, ec_dist=0, min_dev=1.5))
    for mode in (1, 3, 4):
        field = _disturb(oracle.generate(blobs, mode, w, h, xf(fb, -1, 3), overlap=False, ec_mode=0), .25)
        same("distanceSignCorrection%d/zero.25/odd/blobs/40x32" % mode, oracle.sign_correction(blobs, field, xf(fb, -1, 3), .25, 1))
    field = _disturb(oracle.generate(blobs, 3, w, h, xf(fb, -3, 1), overlap=False, ec_mode=0), .75)
    same("distanceSignCorrection3/zero.75/negative/blobs/40x32", oracle.sign_correction(blobs, field, xf(fb, -3, 1), .75, 3))
    same("rasterize/legacy/positive/blobs/40x32", oracle.rasterize(blobs, w, h, xf(fb, 0, 0), 2))
    sdf3 = oracle.generate(a, 3, w, h, xf(fa, -2, 2), ec_mode=0)
    same("renderSDF1from3/range/threshold.4/80x64-from-40x32", oracle.render_sdf(sdf3, 80, 64, 1, -2, 2, .4))
    same("renderSDF3from3/inverted/threshold.5/52x29-from-40x32", oracle.render_sdf(sdf3, 52, 29, 3, 2, -1, .5))
    sdf4 = oracle.generate(a, 4, w, h, xf(fa, -2, 2), ec_mode=0)
    same("simulate8bit4/contiguous/40x32", oracle.simulate_8bit(sdf4*np.float32(1.5)-np.float32(.25)))


# ---- the two twins against each other ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_hip_twin_equals_cpu_twin_byte_for_byte(cpu_twin, tmp_path):
    """Every case of the table: the whole backing buffer (padding, gutters, tails, stencils) out of the shim is what msdfgen's own code leaves there."""
    if not os.path.exists(HIP):
        pytest.skip("oracle/_ref/shim_surface_hip not built (needs the msdfgen headers)")
    want, want_meta, want_ids = cpu_twin
    got, got_meta, got_ids = run_twin(HIP, tmp_path)
    assert got_ids == want_ids and len(got_ids) > 400
    assert sorted(got_meta) == sorted(want_meta) and all((got_meta[k].view(np.uint64) == want_meta[k].view(np.uint64)).all() for k in want_meta)
    failures = []
    for case in want_ids:
        (sig_a, a), (sig_b, b) = want[case], got[case]
        assert sig_a == sig_b, case
        if a != b:
            x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
            where = np.flatnonzero(x != y) if len(a) == len(b) else np.array([min(len(a), len(b))])
            failures.append("%s [%s]: %d of %d bytes differ, first at offset %d" % (case, sig_a, len(where), len(a), int(where[0])))
    assert not failures, "%d of %d cases differ:\n%s" % (len(failures), len(want_ids), "\n".join(failures))
