"""What a chain installs into its library context and how it comes out again (shapemol_amd/guidance.py: _resolve_chain,
_ChainSettings), on the host: a recording fake stands in for the library, so no GPU and no built library are needed.
Every setter that a chain called -- also one that failed -- must be followed by its clearing call, with the arguments of CLEAR
(the library's "nothing installed" form of each setter); nothing else is cleared, and nothing is cleared twice."""
import types

import numpy as np
import pytest
import torch

from shapemol_amd import _lib, guidance as G

CTX, DEV = object(), "the-device"
# setter -> the arguments (after the context) that take its setting out of the context again
CLEAR = {"shapemol_set_mesh_guidance_groups": (0, None, None, None, None, None, None, None, 0, None),
         "shapemol_set_guidance_groups": (0, None, None, None, None, 0, None),
         "shapemol_set_option": (b"first_step", 0),
         "shapemol_set_cfg_groups": (0, None, None, 0, 0.0, None, None, None),
         "shapemol_set_cfg": (0.0, 0, 0.0, None, None, None),
         "shapemol_set_field_guidance": (None, 0.0, 0)}
SETS = ("shapemol_set_mesh_guidance_groups", "shapemol_set_guidance_groups")      # cleared by clear_finished, after a synchronise
MODEL = types.SimpleNamespace(cond_mask_prob=0.1, num_timesteps=1000)
VERTS = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
FACES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
CLOUD = np.arange(24.0).reshape(8, 3)


class Boom(Exception):
    pass


class FakeLib:
    """shapemol_set_* record (name, args after the context) and return 0; the fail_at-th installing call returns 1 or raises."""

    def __init__(self, fail_at=None, how="rc"):
        self.calls, self.fail_at, self.how, self.installs = [], fail_at, how, 0

    def shapemol_last_error(self):
        return b"refused by the fake"

    def __getattr__(self, name):
        if not name.startswith("shapemol_set_"):
            raise AttributeError(name)

        def setter(ctx, *args):
            assert ctx is CTX
            self.calls.append((name, args))
            if args != CLEAR[name]:
                self.installs += 1
                if self.installs - 1 == self.fail_at:
                    if self.how == "raise":
                        raise Boom(name)
                    return 1
            return 0
        return setter


def _decoder():
    from shapemol_amd.shape_autoencoder import DecoderInner
    dec = DecoderInner(3, 32, 128, 4, "signeddist")
    dec._context = lambda dev: "decoder-context"
    return dec


def _plan(first_step=3, **kw):
    args = dict(threshold_type=None, threshold_args=None, num_steps=None, center_pos_mode="none", use_grad=False, grad_lr=1,
                shape_AE=None, use_mesh_data=None, use_pointcloud_data=None, grad_step=500, guide_stren=0, bounds=None)
    args.update(kw)
    return G._resolve_chain(MODEL, torch.zeros(2, 96), first_step=first_step, **args)


# kind -> (keyword arguments of a chain of 2 molecules in 2 groups, the setters it calls in order, first_step = 3 included)
PLANS = {
    "none": (dict(), ["shapemol_set_option"]),
    "cloud_groups": (dict(use_pointcloud_data=[(CLOUD, None, 0.2, 1), (CLOUD + 1, None, 0.3, 1)]),
                     ["shapemol_set_guidance_groups", "shapemol_set_option"]),
    "mesh_groups": (dict(use_mesh_data=[((VERTS, FACES), CLOUD, None, 1), ((VERTS, FACES), CLOUD + 1, None, 1)]),
                    ["shapemol_set_mesh_guidance_groups", "shapemol_set_option"]),
    "field": (dict(use_grad=True), ["shapemol_set_option", "shapemol_set_field_guidance"]),
    "cfg_scalar": (dict(guide_stren=0.7, threshold_type="rescale", bounds=np.array([[-1.0, 1.0]] * 3)),
                   ["shapemol_set_option", "shapemol_set_cfg"]),
    "cfg_groups": (dict(guide_stren=[(0.7, 1), (1.5, 1)], threshold_type="rescale"), ["shapemol_set_option", "shapemol_set_cfg_groups"]),
}
CASES = [(kind, k, how) for kind, (_, setters) in PLANS.items() for k in range(len(setters)) for how in ("rc", "raise")]


def _settings(kind):
    kw = dict(PLANS[kind][0])
    if kind == "field":
        kw["shape_AE"] = _decoder()
    draws = torch.zeros(2, 5, 7, dtype=torch.float64) if kind.endswith("_groups") and not kind.startswith("cfg") else None
    return G._ChainSettings(_plan(**kw), {}, draws)


def _chain(settings, lib):
    """The handlers of sample_diffusion and of the chain handle around install and the enqueue."""
    try:
        try:
            settings.install(lib, CTX, DEV)
            lib.calls.append(("shapemol_sample", ()))
        finally:
            settings.clear_enqueued(lib, CTX)
    except BaseException:
        settings.clear_finished(lib, CTX, DEV)       # _PendingChain.abandon()
        raise
    settings.clear_finished(lib, CTX, DEV)           # _PendingChain.result()


@pytest.fixture
def fake(monkeypatch):
    def make(**kw):
        lib = FakeLib(**kw)
        monkeypatch.setattr(_lib, "load", lambda: lib)        # (_lib.check asks the library for the message of a failed call)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: lib.calls.append(("synchronize", (dev,))))
        return lib
    return make


def _check_cleared(calls):
    """Every installing call is followed by exactly one clearing call of its setter, a set's after a synchronise; no other clears."""
    installs = [(i, name) for i, (name, args) in enumerate(calls) if name in CLEAR and args != CLEAR[name]]
    clears = [(i, name) for i, (name, args) in enumerate(calls) if name in CLEAR and args == CLEAR[name]]
    assert sorted(n for _, n in installs) == sorted(n for _, n in clears), calls
    for i, name in installs:
        j = next(j for j, n in clears if n == name)
        assert j > i, calls
        if name in SETS:
            assert calls[j - 1] == ("synchronize", (DEV,)), calls
    assert sum(1 for name, _ in calls if name == "synchronize") == sum(1 for _, n in installs if n in SETS), calls


@pytest.mark.parametrize("kind,k,how", CASES)
def test_a_failed_setter_leaves_nothing_installed(fake, kind, k, how):
    lib, settings = fake(fail_at=k, how=how), _settings(kind)
    with pytest.raises(Boom if how == "raise" else _lib.ShapeMolLibraryError):
        _chain(settings, lib)
    names = [name for name, args in lib.calls if name in CLEAR and args != CLEAR[name]]
    assert names == PLANS[kind][1][:k + 1]               # the setters up to the failing one were called, none behind it
    assert ("shapemol_sample", ()) not in lib.calls
    _check_cleared(lib.calls)
    n = len(lib.calls)
    settings.clear_enqueued(lib, CTX)
    settings.clear_finished(lib, CTX, DEV)
    assert len(lib.calls) == n                           # a second clear issues no call


@pytest.mark.parametrize("kind", list(PLANS))
def test_success_path_installs_enqueues_and_clears_in_order(fake, kind):
    lib, settings = fake(), _settings(kind)
    _chain(settings, lib)
    setters = PLANS[kind][1]
    names = [name for name, _ in lib.calls]
    late = [s for s in setters if s in SETS]
    assert names == setters + ["shapemol_sample"] + [s for s in setters if s not in SETS] + (["synchronize"] + late if late else [])
    _check_cleared(lib.calls)
    n = len(lib.calls)
    settings.clear_enqueued(lib, CTX)
    settings.clear_finished(lib, CTX, DEV)
    assert len(lib.calls) == n


def test_a_chain_without_settings_calls_nothing(fake):
    lib = fake()
    _chain(G._ChainSettings(_plan(first_step=0), {}, None), lib)
    assert lib.calls == [("shapemol_sample", ())]


def test_installed_arguments(fake):
    """What the setters get: group counts, the threshold code and p, the strength, grad_lr and grad_step, the draws pointer."""
    lib, settings = fake(), _settings("cloud_groups")
    _chain(settings, lib)
    args = lib.calls[0][1]
    assert args[0] == 2 and args[5] == 500 and args[6].value == settings.gd.data_ptr()
    lib = fake()
    _chain(_settings("cfg_scalar"), lib)
    assert lib.calls[0] == ("shapemol_set_option", (b"first_step", 3))
    stren, code, p, box, pos_u, v_u = lib.calls[1][1]
    assert (stren, code, p, pos_u, v_u) == (0.7, 3, 0.7, None, None) and box is not None
    lib = fake()
    _chain(_settings("cfg_groups"), lib)
    assert lib.calls[1][1][0] == 2 and lib.calls[1][1][3:5] == (3, 0.7) and lib.calls[1][1][5] is None
    lib = fake()
    _chain(_settings("field"), lib)
    assert lib.calls[1] == ("shapemol_set_field_guidance", ("decoder-context", 1.0, 500))


@pytest.mark.parametrize("mesh,cloud,field,cfg", [(m, c, f, g) for m in (0, 1) for c in (0, 1) for f in (0, 1) for g in (0, 1)])
def test_resolve_chain_precedence(mesh, cloud, field, cfg):
    """The reference's if / elif over what is given: mesh > point cloud > gradient field > classifier-free guidance > none."""
    dec = _decoder()
    plan = _plan(first_step=0, use_mesh_data=((VERTS, FACES), CLOUD, None) if mesh else None,
                 use_pointcloud_data=(CLOUD, None, 0.2) if cloud else None, use_grad=bool(field), shape_AE=dec if field else None,
                 guide_stren=0.7 if cfg else 0, threshold_type="rescale" if cfg else None)
    want = "mesh_groups" if mesh else "groups" if cloud else "field" if field else "cfg" if cfg else None
    assert plan.kind == want
    assert (plan.field_dec is dec) == (want == "field") and (plan.field_dec is None) == (want != "field")
    assert plan.num_steps == 1000 and plan.first_step == 0 and plan.center_pos_mode == "none"
    if want in ("mesh_groups", "groups"):            # the tuple form: one group, once the batch is known
        assert plan.payload is None and plan.n_mesh_groups == 0
        plan.one_group(2)
        assert plan.payload[0].tolist() == [0, 2]
