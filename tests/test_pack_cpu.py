"""The device weight image built by csrc/sm_pack.h, without a GPU.

tests/pack_probe.cpp includes sm_pack.h, builds the image of a model's packed weights and reports its size, hid_max and every
DevModel / DevLayer offset; the image bytes are hashed here.  The expected values (tests/golden/pack_image.json) were recorded
with this same probe from the packer as it stood before it was restructured (the code moved into sm_pack.h verbatim).
UPDATE_PACK_GOLDEN=1 rewrites the fixture."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from util import GOLDEN, ROOT, model_cfg, synth

FIXTURE = os.path.join(GOLDEN, "pack_image.json")
CASES = {
    "full": dict(),                                             # the sampling model: H = 128, k as configured
    "reduced_h32": dict(hidden_dim=32, n_heads=4, num_layers=2),     # the reduced model of the GPU tests
    "k32": dict(knn=32, num_layers=2),
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("pack_probe") / "pack_probe")
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O2", "-o", exe,
                        os.path.join(ROOT, "tests", "pack_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def run_probe(exe, overrides, tmp_path):
    from shapemol_amd import _lib, pack_state_dict
    from shapemol_amd.spec import ModelDims
    cfg = model_cfg(**overrides)
    d = ModelDims(cfg, 15)
    packed = pack_state_dict(synth.synthetic_state_dict(cfg, seed=7), d.L)
    conf = _lib.Config(d.H, d.heads, d.L, d.k, d.G, d.S, d.S_latent, d.temb, d.C, d.T)
    src, dst = str(tmp_path / "weights.bin"), str(tmp_path / "image.bin")
    with open(src, "wb") as f:
        f.write(bytes(conf))
        f.write(np.ascontiguousarray(packed, np.float32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split() for line in r.stdout.splitlines())
    image = open(dst, "rb").read()
    assert len(image) == 4 * int(out["size"])
    out["sha256"] = hashlib.sha256(image).hexdigest()
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_image_is_what_the_packer_always_built(probe, case, tmp_path):
    got = run_probe(probe, CASES[case], tmp_path)
    if os.environ.get("UPDATE_PACK_GOLDEN") == "1":
        all_ = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}
        all_[case] = got
        json.dump(all_, open(FIXTURE, "w"), indent=0, sort_keys=True)
    want = json.load(open(FIXTURE))[case]
    assert sorted(got) == sorted(want)
    assert len(got) > 100                    # every offset is reported
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff
