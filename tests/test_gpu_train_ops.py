"""The training step's four device operators (shapemol_amd/training.py: HipMLP, HipEdgeMLP, HipSegAttention, HipVN; kernels
csrc/sm_train.h, host code csrc/train_ops.hip) against the float64 oracle (tests/train_ops_f64.py) under the project's gate
eH <= 4 e32 + 16 * 2^-24 per tensor, at the tile, split and alignment edges of tests/train_ops_cases.py (which
tests/test_train_ops_cpu.py proves well-posed); the branches of the C ABI that no Python caller takes (d_act == NULL,
d_dx == NULL, operands off the 16-byte alignment), every output and workspace prefilled with NaN; the host-side refusals."""
import ctypes as C

import pytest
import torch

import train_ops_cases as TC
import train_ops_f64 as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CASES = [(kind, case) for kind, cases in TC.ALL.items() for case in cases]
IDS = [kind + "-" + TC.case_id(case) for kind, case in CASES]


def _lib():
    from shapemol_amd import _lib as L
    return L.load()


def _stream():
    from shapemol_amd._native import stream_ptr
    return stream_ptr(torch.device(DEV))


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _grad(t):
    return (t.grad if t.grad is not None else torch.zeros_like(t)).cpu()      # (autograd may leave a leaf without entries alone)


# ------------------------------------------------------------------------------------------------------------------------
# the autograd wrappers, once per call: {tensor name: CPU tensor}
# ------------------------------------------------------------------------------------------------------------------------
def _graph(inp):
    from shapemol_amd.training import EdgeGraph
    return EdgeGraph(inp["src"].to(DEV), inp["dst"].to(DEV), inp["ptr"].to(DEV))


def run_wrapper(kind, case):
    from shapemol_amd import training as T
    inp = TO.evaluate(kind, case)[0]
    if kind == "mlp":
        a = [_leaf(t) for t in [inp["x"]] + inp["ws"]]
        out = T.HipMLP.apply(*a)
        out.backward(inp["dy"].to(DEV))
        names = TO.MLP_OUT
    elif kind == "edge":
        a = [_leaf(t) for t in [inp["r"], inp["h"], inp["s"]] + inp["ws"]]
        out = T.HipEdgeMLP.apply(a[0], a[1], a[2], _graph(inp), *a[3:])
        out.backward(inp["dy"].to(DEV))
        names = TO.EDGE_OUT
    elif kind == "attn":
        a = [_leaf(t) for t in (inp["q"], inp["k"], inp["vals"])]
        out = T.HipSegAttention.apply(a[0], a[1], a[2], inp["ptr"].to(DEV), case.heads)
        out.backward(inp["dout"].to(DEV))
        names = TO.ATTN_OUT
    else:
        a = [_leaf(t) for t in [inp["x"], inp["o3"]] + inp["ws"]]
        rm, rv = inp["run_mean"].to(DEV).clone(), inp["run_var"].to(DEV).clone()
        out = T.HipVN.apply(a[0], a[1], inp["shape"].to(DEV), inp["batch"].to(DEV), a[2], a[3], a[4], a[5], rm, rv, case.training)
        out.backward(inp["gout"].to(DEV))
        res = dict(zip(TO.VN_OUT, [out.detach().cpu()] + [_grad(t) for t in a]))
        res["run_mean"], res["run_var"] = rm.cpu(), rv.cpu()
        return res
    return dict(zip(names, [out.detach().cpu()] + [_grad(t) for t in a]))


def workspace_floats(kind, case):
    lib = _lib()
    if kind == "mlp":
        return int(lib.shapemol_mlp_backward_workspace(case.rows, case.k_in, case.hidden, case.n_out))
    if kind == "edge":
        E = TO.evaluate(kind, case)[0]["src"].numel()
        return int(lib.shapemol_edge_mlp_backward_workspace(E, case.n_atoms, case.k_edge, case.k_node, case.k_shape, case.hidden, case.n_out))
    if kind == "vn":
        return int(lib.shapemol_vn_backward_workspace(case.atoms, case.rows_o, case.rows_s, case.C))
    return 0


def poison(sizes):
    """Blocks of the given sizes filled with NaN and handed back to the caching allocator: what the next torch.empty of such a
    size receives.  (Without it the second run of a shape receives the first run's results: the right answer.)"""
    blocks = [torch.full((max(int(n), 1),), NAN, dtype=torch.float32, device=DEV) for n in sizes]
    torch.cuda.synchronize()
    del blocks


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_gate(kind, case):
    from util import record
    _, r32, r64, bad, _ = TO.evaluate(kind, case)
    assert bad == 0
    res = run_wrapper(kind, case)
    zero = TC.zero_by_construction(kind, case)
    for key in zero:
        assert float(res[key].abs().max()) == 0.0, key
    gates = TO.gate(res, r32, r64, skip=zero)
    name = kind + "-" + TC.case_id(case)
    ok = TO.report(name, gates)
    key, ratio = TO.worst(gates)
    record("train_ops_gate", case=name, worst=key, eH=gates[key][0], e32=gates[key][1], bound=gates[key][2], ratio=ratio)
    assert ok, {k: g for k, g in gates.items() if not g[3]}
    if kind == "vn" and not case.training:      # evaluation mode leaves the running statistics alone, bit for bit
        inp = TO.evaluate(kind, case)[0]
        assert torch.equal(res["run_mean"], inp["run_mean"]) and torch.equal(res["run_var"], inp["run_var"])
    # the same case again, with NaN where the allocator will place the workspace, the saved activations and the outputs
    sizes = [workspace_floats(kind, case)] + [t.numel() for t in res.values()]
    if kind in ("mlp", "edge"):
        sizes += [res["y"].shape[0] * case.hidden] * 3
    poison(sizes + sizes)
    again = run_wrapper(kind, case)
    for k, t in res.items():
        assert bool(torch.isfinite(again[k]).all()), k
        assert torch.equal(again[k], t), k


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI directly, as training.py calls it: every buffer a slice of a NaN-filled block, `off` floats behind its start
# ------------------------------------------------------------------------------------------------------------------------
def _buf(n, off=0):
    return torch.full((n + off + 4,), NAN, dtype=torch.float32, device=DEV)[off:off + n]


def _put(t, off=0):
    b = _buf(t.numel(), off)
    b.copy_(t.reshape(-1).to(DEV))
    return b


def _p(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def mlp_abi(case, off=0, act_null=False, dx_null=False):
    lib, inp = _lib(), TO.evaluate("mlp", case)[0]
    R, K, H, O = case.rows, case.k_in, case.hidden, case.n_out
    x, dy = _put(inp["x"], off), _put(inp["dy"], off)
    w1, b1, ga, be, w2, b2 = [_put(t, off) for t in inp["ws"]]
    y, xhat, rstd, act = _buf(R * O, off), _buf(R * H, off), _buf(R, off), _buf(R * H, off)
    with torch.cuda.device(0):
        assert lib.shapemol_mlp_forward(_p(x), R, K, H, O, _p(w1), _p(b1), _p(ga), _p(be), _p(w2), _p(b2), _p(y), _p(xhat), _p(rstd), _p(act), _stream()) == 0
        n_work = int(lib.shapemol_mlp_backward_workspace(R, K, H, O))
        work = _buf(n_work, off)
        g = dict(dx=_buf(R * K, off), dW1=_buf(H * K, off), db1=_buf(H, off), dgamma=_buf(H, off), dbeta=_buf(H, off), dW2=_buf(O * H, off), db2=_buf(O, off))
        rc = lib.shapemol_mlp_backward(_p(x), _p(dy), R, K, H, O, _p(w1), _p(ga), _p(be), _p(w2), _p(xhat), _p(rstd), None if act_null else _p(act),
                                       None if dx_null else _p(g["dx"]), _p(g["dW1"]), _p(g["db1"]), _p(g["dgamma"]), _p(g["dbeta"]), _p(g["dW2"]), _p(g["db2"]),
                                       _p(work), n_work, _stream())
        assert rc == 0, lib.shapemol_last_error()
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(y=y, **g).items()}


def edge_abi(case, off=0, act_null=False):
    lib, inp = _lib(), TO.evaluate("edge", case)[0]
    gr = _graph(inp)
    E, N, kr, kn, ks, H, O = gr.E, gr.n, case.k_edge, case.k_node, case.k_shape, case.hidden, case.n_out
    K1 = kr + 2 * kn + ks
    r, h, s, dy = _put(inp["r"], off), _put(inp["h"], off), _put(inp["s"], off), _put(inp["dy"], off)
    w1, b1, ga, be, w2, b2 = [_put(t, off) for t in inp["ws"]]
    y, xhat, rstd, act, pd, ps = _buf(E * O, off), _buf(E * H, off), _buf(E, off), _buf(E * H, off), _buf(N * H, off), _buf(N * H, off)
    with torch.cuda.device(0):
        rc = lib.shapemol_edge_mlp_forward(_p(r), _p(h), _p(s), _p(gr.dst), _p(gr.src), E, N, kr, kn, ks, H, O, _p(w1), _p(b1), _p(ga), _p(be), _p(w2), _p(b2),
                                           _p(y), _p(xhat), _p(rstd), _p(act), _p(pd), _p(ps), _stream())
        assert rc == 0, lib.shapemol_last_error()
        n_work = int(lib.shapemol_edge_mlp_backward_workspace(E, N, kr, kn, ks, H, O))
        work = _buf(n_work, off)
        g = dict(dr=_buf(E * kr, off), dh=_buf(N * kn, off), ds=_buf(N * ks, off), dW1=_buf(H * K1, off), db1=_buf(H, off), dgamma=_buf(H, off),
                 dbeta=_buf(H, off), dW2=_buf(O * H, off), db2=_buf(O, off))
        rc = lib.shapemol_edge_mlp_backward(_p(r), _p(h), _p(s), _p(gr.ptr), _p(gr.perm_src), _p(gr.ptr_src), _p(dy), E, N, kr, kn, ks, H, O, _p(w1), _p(ga), _p(be),
                                            _p(w2), _p(xhat), _p(rstd), None if act_null else _p(act), _p(g["dr"]), _p(g["dh"]), _p(g["ds"]), _p(g["dW1"]),
                                            _p(g["db1"]), _p(g["dgamma"]), _p(g["dbeta"]), _p(g["dW2"]), _p(g["db2"]), _p(work), n_work, _stream())
        assert rc == 0, lib.shapemol_last_error()
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dict(y=y, **g).items()}


def _same_bits(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k


def _mlp_case(rows, k_in):
    return next(c for c in TC.MLP if (c.rows, c.k_in) == (rows, k_in))


def _edge_case(widths=None, n_edges=None):
    return next(c for c in TC.EDGE if (c.k_edge, c.k_node, c.k_shape) == widths or (n_edges is not None and c.n_edges == n_edges))


ABI_MLP = [_mlp_case(513, 8), _mlp_case(8449, 4), _mlp_case(33, 20)]       # ragged split; real_splits < row_splits; K tail on float4
ABI_EDGE = [_edge_case(widths=(4, 6, 4)), _edge_case(n_edges=513)]          # partial float4 in N; edge and node split counts differ


@pytest.mark.parametrize("case", ABI_MLP, ids=TC.case_id)
def test_mlp_abi_branches(case):
    ref = run_wrapper("mlp", case)
    base = mlp_abi(case)
    # (a) outputs and workspace were NaN: every entry was written, and with the wrapper's bits
    assert all(bool(torch.isfinite(t).all()) for t in base.values())
    _same_bits(base, ref)
    # (b) d_act == NULL: relu_affine_kernel recomputes the forward's activation
    _same_bits(mlp_abi(case, act_null=True), base)
    # (c) d_dx == NULL: the six parameter gradients are untouched by it, dx is not written
    nodx = mlp_abi(case, dx_null=True)
    _same_bits(nodx, base, ("y", "dW1", "db1", "dgamma", "dbeta", "dW2", "db2"))
    assert bool(torch.isnan(nodx["dx"]).all())
    # (d) every operand one float off the 16-byte alignment: gemm() takes the scalar kernel, which zero-pads alike and runs the
    # same MFMA sequence
    _same_bits(mlp_abi(case, off=1), base)
    _same_bits(mlp_abi(case, off=1, act_null=True), base)


@pytest.mark.parametrize("case", ABI_EDGE, ids=TC.case_id)
def test_edge_abi_branches(case):
    ref = run_wrapper("edge", case)
    base = edge_abi(case)
    assert all(bool(torch.isfinite(t).all()) for t in base.values())
    _same_bits(base, ref)
    _same_bits(edge_abi(case, act_null=True), base)
    _same_bits(edge_abi(case, off=1), base)


def test_workspace_sizes_imply_the_expected_split_counts():
    """(e) The split count the library carves its workspace by, from shapemol_mlp_backward_workspace minus the terms that do not
    depend on it (train_ops.hip:77-81), for every MLP case; the edge form's and the VN block's totals from the cases' counts."""
    lib = _lib()
    for c in TC.MLP:
        total = int(lib.shapemol_mlp_backward_workspace(c.rows, c.k_in, c.hidden, c.n_out))
        rest = total - 64 - 2 * c.rows * c.hidden - c.blocks * (3 * c.hidden + c.n_out)
        per_split = c.hidden * c.k_in + c.n_out * c.hidden
        assert rest % per_split == 0 and rest // per_split == c.splits, c
    for c in TC.EDGE:
        E = TO.evaluate("edge", c)[0]["src"].numel()
        blocks = -(-E // 64)
        part = max(c.splits_e * c.n_out * c.hidden, c.splits_e * c.hidden * c.k_edge, c.splits_n * c.hidden * max(c.k_node, c.k_shape))
        assert workspace_floats("edge", c) == 2 * E * c.hidden + 2 * c.n_atoms * c.hidden + part + blocks * (3 * c.hidden + c.n_out) + 64, c
    for c in TC.VN:
        assert workspace_floats("vn", c) == 9 * c.atoms * c.C + 2 * c.C + c.blocks * 2 * c.C * (1 + c.rows_o + c.rows_s) + 64, c


# ------------------------------------------------------------------------------------------------------------------------
# refusals: host-side returns, nothing is launched, the buffers stay as prefilled
# ------------------------------------------------------------------------------------------------------------------------
def _call(fn, ints, buf, size=None):
    """fn with `buf` for every pointer argument, the integer arguments from `ints` in order, `size` for the size_t one."""
    it, args = iter(ints), []
    for t in fn.argtypes[:-1]:
        args.append(C.c_void_p(buf.data_ptr()) if t is C.c_void_p else size if t is C.c_size_t else next(it))
    assert next(it, None) is None
    with torch.cuda.device(0):
        return fn(*args, _stream())


def test_refusals():
    lib = _lib()
    buf = torch.full((1 << 20,), 7.0, dtype=torch.float32, device=DEV)       # (far larger than any operand of these shapes)
    err = lambda: lib.shapemol_last_error().decode()  # noqa: E731
    ws_mlp = lambda *d: int(lib.shapemol_mlp_backward_workspace(*d))  # noqa: E731
    # MLP and edge form: hidden above the LDS limit of the LayerNorm backward, no rows
    for dims in ((4, 8, 257, 8), (0, 8, 8, 8)):
        assert ws_mlp(*dims) == 0
        assert _call(lib.shapemol_mlp_forward, dims, buf) == 1 and "out of range" in err()
        assert _call(lib.shapemol_mlp_backward, dims, buf, size=1 << 20) == 1 and "out of range" in err()
    for dims in ((4, 3, 4, 8, 4, 257, 8), (0, 3, 4, 8, 4, 8, 8)):
        assert int(lib.shapemol_edge_mlp_backward_workspace(*dims)) == 0
        assert _call(lib.shapemol_edge_mlp_forward, dims, buf) == 1 and "out of range" in err()
        assert _call(lib.shapemol_edge_mlp_backward, dims, buf, size=1 << 20) == 1 and "out of range" in err()
    # segment attention: dh, W above 8
    for dims in ((4, 2, 9, 3), (4, 2, 8, 9)):
        assert _call(lib.shapemol_seg_attention_forward, dims, buf) == 1 and "out of range" in err()
        assert _call(lib.shapemol_seg_attention_backward, dims, buf) == 1 and "out of range" in err()
    # VN: more than 64 channels; a weight block 2 C (1 + rows_o + rows_s) floats above 48 KB (64 x 97 x 2 x 4 = 49 664 bytes)
    for dims in ((8, 3, 4, 65), (8, 0, 96, 64)):
        assert int(lib.shapemol_vn_backward_workspace(*dims)) == 0
        assert _call(lib.shapemol_vn_forward, dims + (1,), buf) == 1 and "out of range" in err()
        assert _call(lib.shapemol_vn_backward, dims + (1,), buf, size=1 << 20) == 1 and "out of range" in err()
    assert int(lib.shapemol_vn_backward_workspace(8, 0, 95, 64)) > 0                # 49 152 bytes: the limit itself is accepted
    # a workspace one float short of what the workspace function asks for
    dims = (70, 8, 8, 8)
    assert _call(lib.shapemol_mlp_backward, dims, buf, size=ws_mlp(*dims) - 1) == 1 and "workspace too small" in err()
    dims = (70, 9, 4, 8, 4, 8, 8)
    assert _call(lib.shapemol_edge_mlp_backward, dims, buf, size=int(lib.shapemol_edge_mlp_backward_workspace(*dims)) - 1) == 1 and "workspace too small" in err()
    dims = (8, 3, 4, 16)
    assert _call(lib.shapemol_vn_backward, dims + (1,), buf, size=int(lib.shapemol_vn_backward_workspace(*dims)) - 1) == 1 and "workspace too small" in err()
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


def test_wrappers_pass_operands_of_zero_rows():
    """rows_o == 0 and rows_s == 0 go through HipVN (null pointers for the operands without entries), k_shape == 0 through
    HipEdgeMLP: the gradients of those operands are tensors without entries."""
    res = run_wrapper("vn", next(c for c in TC.VN if c.rows_o == 0))
    assert res["do3"].shape[1:] == (0, 3) and bool(torch.isfinite(res["dx"]).all())
    res = run_wrapper("edge", next(c for c in TC.EDGE if c.k_shape == 0))
    assert res["ds"].shape[1] == 0
