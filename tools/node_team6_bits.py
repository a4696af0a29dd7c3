"""Bit equality of the exact-mode node kernels between two builds of the library (profiles/node_team6/).

    python tools/node_team6_bits.py [--libs parent,] [--out bit_equality.txt]

One fresh child process per library (SHAPEMOL_LIB=<name>, "" = the tree's own build); every case runs twice per library.  A
line per (case, tensor): the sha256 (16 hex digits) of the four runs and a verdict -- `equal`, `DIFFERENT`, or `parent-unstable`
when the first library does not agree with itself.  The launch records of a case are printed and compared too.
Exit status 1 if any tensor on which the first library agrees with itself differs in the second.
Cases: the sizes of tests/test_gpu_node_levels.py in both node-stage forms, the mode variants that change which node kernel
runs, the golden forward batches, and 20-step chains; full model (2 layers) and the reduced one."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"node_levels": 1, "after_order": 2, "after_waves": 16, "stop_layer": -1, "prologue_tab": 1, "x2h_out_fuse": 1,
            "edge_bf16": 2, "node_f16": 0}
MODELS = {"full": dict(num_layers=2), "reduced": dict(hidden_dim=32, n_heads=4, num_layers=2)}
SIZES = (1, 15, 16, 17, 31, 32, 33, 49)


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import chain_forms as CF
    from test_gpu_node_levels import _counts
    from util import T, golden, hash_noise, hip_model, synth
    dev = "cuda:0"

    def emit(case, run, tensors, records):
        print(json.dumps(dict(case=case, run=run, sha={k: sha(v) for k, v in tensors.items()}, rec=records)), flush=True)

    def with_options(m, opts, fn):
        try:
            for k, v in opts.items():
                m.set_option(k, v)
            return fn()
        finally:
            for k in opts:
                m.set_option(k, DEFAULTS[k])

    def forward(m, h, pos, v, batch, shape, t, taps=True):
        n = len(batch)
        with torch.no_grad():
            out = m(T(pos, dev), T(v, dev), T(batch, dev), T(shape, dev), T(t, dev))
        got = {k: out[k].cpu().numpy() for k in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")}
        if taps:
            got["q"] = m.debug_read("q", (n, h), np.float32)
            got["q_x"] = m.debug_read("q_x", (n, h), np.float32)
            got["pre"] = m.debug_read("pre", (n, 8 * h), np.float32)
        rec = {"launch_node": m.debug_read("launch_node", (8,), np.int64).tolist()}
        return got, rec

    def sized(m, h, n):
        bb = CF.batch(_counts(n), seed=11)
        t = (np.arange(len(bb["counts"]), dtype=np.int64) * 377 + 123) % 1000
        return forward(m, h, bb["init_pos"], bb["init_v"], bb["batch"], bb["shape"], t)

    for name, ov in MODELS.items():
        m, h = hip_model(**ov), ov.get("hidden_dim", 128)
        cases = []
        for n in SIZES:
            for lv in (1, 0):
                cases.append((f"fwd/{name}/n{n}/levels{lv}", {"node_levels": lv}, n))
        for lv in (1, 0):
            cases.append((f"fwd/{name}/n33/levels{lv}/stop1", {"node_levels": lv, "stop_layer": 1}, 33))
        for order in (0, 1):
            cases.append((f"fwd/{name}/n49/waves8/order{order}", {"after_waves": 8, "after_order": order}, 49))
        for n in (17, 49):
            for opt in ("prologue_tab", "x2h_out_fuse"):
                for val in (0, 1):
                    cases.append((f"fwd/{name}/n{n}/{opt}{val}", {opt: val}, n))
            cases.append((f"fwd/{name}/n{n}/f16_edges_exact_nodes", {"edge_bf16": 3, "node_f16": 0}, n))
        for case, opts, n in cases:
            for run in (0, 1):
                got, rec = with_options(m, opts, lambda: sized(m, h, n))
                if "stop_layer" in opts:
                    got["pre"] = got["pre"][:, :4 * h]      # (the other half is not written by a one-layer evaluation)
                emit(case, run, got, rec)
        f = golden("forward_b4.npz")
        g = golden("forward_ragged.npz")
        for run in (0, 1):
            emit(f"fwd/{name}/golden_b4", run, *forward(m, h, f["pos"], f["v"], f["batch"], f["shape"], f["t500_t"]))
            emit(f"fwd/{name}/golden_ragged", run, *forward(m, h, g["pos"], g["v"], g["batch"], g["shape"], g["t"]))

    def chain(m, bb, steps, eps, u):
        b = len(bb["shape"])
        r = m.sample_diffusion(T(bb["init_pos"], dev), T(bb["init_v"], dev), T(bb["batch"], dev), T(bb["shape"], dev).view(b, -1),
                               num_steps=steps, center_pos_mode="none", noise=(T(eps, dev), T(u, dev)))
        got = {"pos": r["pos"].cpu().numpy(), "v": r["v"].cpu().numpy(),
               "pos_traj": torch.stack(r["pos_traj"]).cpu().numpy(), "v_traj": torch.stack(r["v_traj"]).cpu().numpy()}
        rec = {"launch": m.debug_read("launch", (8,), np.int64).tolist(), "launch_node": m.debug_read("launch_node", (8,), np.int64).tolist()}
        return got, rec

    steps = 20
    chains = [(f"chain/{name}/{tag}", ov, 15, opts) for name, ov in MODELS.items() for tag, opts in (
        ("default", {}), ("prologue_tab0", {"prologue_tab": 0}), ("levels0", {"node_levels": 0}),
        ("levels0_prologue_tab0", {"node_levels": 0, "prologue_tab": 0}))]
    chains.append(("chain/full/c23", MODELS["full"], 23, {}))
    for case, ov, C, opts in chains:
        m = hip_model(num_classes=C, **ov)
        bb = synth.synthetic_batch(4, seed=9, num_classes=C)
        eps, u = hash_noise(len(bb["batch"]), steps, 9, c=C)
        for run in (0, 1):
            emit(case, run, *with_options(m, opts, lambda: chain(m, bb, steps, eps, u)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--libs", default="parent,", help="comma-separated SHAPEMOL_LIB names; the empty name is the tree's own build")
    ap.add_argument("--out", default="bit_equality.txt", help="the table (relative to the current directory)")
    a = ap.parse_args()
    if a.child:
        return child()
    libs = a.libs.split(",")
    assert len(libs) == 2
    runs = {}          # lib -> case -> run -> line
    for lib in libs:
        env = dict(os.environ, SHAPEMOL_LIB=lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"library '{lib or 'branch'}': child ended with status {p.returncode}; nothing further is run")
            return 2
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                runs.setdefault(lib, {}).setdefault(d["case"], {})[d["run"]] = d
    names = [l or "branch" for l in libs]
    out, bad, unstable, n_t = [f"# case tensor {names[0]}:run0 {names[0]}:run1 {names[1]}:run0 {names[1]}:run1 verdict"], 0, 0, 0
    for case, r0 in runs[libs[0]].items():
        r1 = runs[libs[1]][case]
        recs = [r0[0]["rec"], r0[1]["rec"], r1[0]["rec"], r1[1]["rec"]]
        same_rec = all(r == recs[0] for r in recs)
        out.append(f"{case} launch-record {json.dumps(recs[0])} {'equal' if same_rec else 'DIFFERENT ' + json.dumps(recs[2])}")
        bad += not same_rec
        for k in r0[0]["sha"]:
            s = [r0[0]["sha"][k], r0[1]["sha"][k], r1[0]["sha"][k], r1[1]["sha"][k]]
            n_t += 1
            if s[0] != s[1]:
                verdict = "parent-unstable"
                unstable += 1
            elif s[2] == s[0] and s[3] == s[0]:
                verdict = "equal"
            else:
                verdict = "DIFFERENT"
                bad += 1
            out.append(f"{case} {k} {' '.join(s)} {verdict}")
    out.append(f"# {len(runs[libs[0]])} cases, {n_t} tensors, {bad} different, {unstable} on which {names[0]} does not agree with itself")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(l for l in out if "DIFFERENT" in l or "unstable" in l or l.startswith("#")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
