"""nn.DataParallel replicas of the mirror modules, without a GPU.

``DataParallel.forward`` calls torch's ``replicate()`` on every forward once more than one device is given (even for a batch of one scene).  A replica has
``_parameters == {}`` (its parameters are plain attributes holding the broadcast copies) and an empty ``state_dict()``; it is a new object, with new
tensors, on every forward.  Pinned here with torch's real ``replicate()`` (broadcast patched to clones, tests/dp_util.py) and the oracle-backed CPU stand-ins
of the ops layer (tests/fake_ops.py): the replicas read their parameters, their packed operands are byte-identical to the source's, they come from ONE
cache shared with the source (a second round packs nothing; an in-place update of the source re-packs once), and copies / pickles / state dicts of the
source are unaffected."""
import copy
import importlib
import os
import pickle
import types

import numpy as np
import pytest
import torch

from dp_util import MiniTrainer, build_reference_trainer, make_networks, make_sample, pack_delta, recon, reference_trainer, replicate_clones

featurenet = importlib.import_module("one-2-3-45_amd.featurenet")
packs = importlib.import_module("one-2-3-45_amd.recon.packs")
D = 14


@pytest.fixture()
def fake(monkeypatch):
    import fake_ops
    fake_ops.install(monkeypatch)


def _bytes(t):
    if isinstance(t, (tuple, list)):
        return b"".join(_bytes(x) for x in t)
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def _sdf_network(lod):
    _, sdf, _, _ = make_networks(D)
    if lod == 0:
        return sdf
    torch.manual_seed(4)
    return recon.SparseSdfNetwork(lod=1, ch_in=56, voxel_size=2.0 / (D - 1), vol_dims=[D, D, D], regnet_d_out=16)


def _operands(mod):
    """Every packed operand of a mirror module, as tensors, in a fixed order."""
    if isinstance(mod, recon.SparseSdfNetwork):
        cr = mod._costreg(torch.device("cpu"))
        out = [mod.sdf_layer.blob(), mod.sdf_layer.grid_tables(8), mod._voxel_lattice((D, D, D), torch.device("cpu")), mod.compress_layer.packed()]
        for name in sorted(cr.p):
            out += list(cr.p[name]) + ([cr.xblob[name]] if name in cr.xblob else [])
        return out
    if isinstance(mod, recon.GeneralRenderingNetwork):
        return list(mod._blobs())
    if isinstance(mod, featurenet.FeatureNet):
        return [m.packed() for m in mod.modules() if isinstance(m, featurenet.ConvBnReLU)] + \
               [featurenet._cached_conv_pack(mod, n, mod.precision) for n in ("toplayer", "smooth1", "smooth0")]
    return []


def _params(mod, like=None):
    """The module's parameters through packs.param, in a fixed order (``like``: the source module, whose tables name them for a replica)."""
    if isinstance(mod, recon.SparseSdfNetwork):
        cl = mod.compress_layer
        return mod.sdf_layer._params() + list(mod._costreg_params(mod).values()) + [packs.param(cl.conv, "weight")] + \
            [packs.param(cl.bn, n) for n in ("weight", "bias")]
    if isinstance(mod, recon.GeneralRenderingNetwork):
        return mod._params()
    if isinstance(mod, recon.SingleVarianceNetwork):
        return [packs.param(mod, "variance")]
    return [packs.param(m, n) for m, s in zip(mod.modules(), (like or mod).modules()) for n, v in s._parameters.items() if v is not None]


MODULES = {"sdf_lod0": lambda: _sdf_network(0), "sdf_lod1": lambda: _sdf_network(1), "rendering": lambda: make_networks(D)[2],
           "variance": lambda: make_networks(D)[3], "featurenet": lambda: make_networks(D)[0]}


@pytest.mark.parametrize("name", sorted(MODULES))
def test_replicas_read_parameters_and_share_one_pack_cache(fake, name):
    src = MODULES[name]()
    keys = list(src.state_dict())
    ref = [_bytes(t) for t in _operands(MODULES[name]())]                     # packed by an independent, identically seeded module
    reps = replicate_clones(src, 2)
    pnames = {n for n, _ in src.named_parameters()}
    assert pnames and all(not (set(r.state_dict()) & pnames) for r in reps)      # what broke the mirrors: no parameter keys, _parameters == {}
    for r in reps:
        assert len(_params(r, src)) == len(pnames)
        assert [_bytes(p) for p in _params(r, src)] == [_bytes(p) for p in _params(src)]
        assert all(a is not b for a, b in zip(_params(r, src), _params(src)))    # the replica's own broadcast copies
    before = recon.pack_stats()
    got = [[_bytes(t) for t in _operands(r)] for r in reps]
    assert got[0] == ref and got[1] == ref
    first = pack_delta(before)
    nconv = {"featurenet": 11, "sdf_lod0": 1, "sdf_lod1": 1}.get(name, 0)
    assert all(v == (nconv if k[0] == "conv" else 1) for k, v in first.items()) and len(first) == len({k[0] for k in first}), first
    assert {k[0] for k in first} == {"featurenet": {"conv"}, "rendering": {"colour"}, "variance": set()}.get(
        name, {"sdf_blob", "sdf_grid", "lattice", "conv", "costreg"}), first
    # a second replicate-and-call round (DataParallel.forward's next call: new replica objects, new tensors) packs nothing
    before = recon.pack_stats()
    for r in replicate_clones(src, 2):
        assert [_bytes(t) for t in _operands(r)] == ref
    assert pack_delta(before) == {}
    # an in-place update of ONE source parameter re-packs exactly once (on the one device), for both replicas
    ps = _params(src)
    if ps and _operands(src):
        with torch.no_grad():
            ps[0].add_(1)
        before = recon.pack_stats()
        outs = [[_bytes(t) for t in _operands(r)] for r in replicate_clones(src, 2)]
        d = pack_delta(before)
        assert sum(d.values()) >= 1 and all(v == 1 for v in d.values()), d
        fresh = MODULES[name]()
        with torch.no_grad():
            _params(fresh)[0].add_(1)
        assert outs[0] == outs[1] == [_bytes(t) for t in _operands(fresh)] != ref
    # the source module itself: state-dict keys, .to(), deepcopy, pickle
    assert list(src.state_dict()) == keys and not any("_packs" in k for k in keys)
    cache = src.__dict__.get("_packs")
    assert src.to("cpu").__dict__.get("_packs") is cache
    for how in (copy.deepcopy, lambda m: pickle.loads(pickle.dumps(m))):
        try:
            cp = how(src)
        except RuntimeError as e:                 # torch's own limit for modules with nn.utils.weight_norm (the SDF layers), as before this cache
            assert "weight_norm" in str(e) and name.startswith("sdf")
            continue
        assert list(cp.state_dict()) == keys
        assert all(torch.equal(a, b) for a, b in zip(cp.state_dict().values(), src.state_dict().values()))
        if cache is not None:
            assert cp._packs is not cache and len(cp._packs) == 0 and cp._packs.owner() is cp
    if cache is not None:
        featurenet.invalidate_packed(src)
        assert len(cache) == 0


def test_state_dict_keys_are_the_references(fake):
    feat, sdf, ren, var = make_networks(D)
    assert len(ren.state_dict()) == 23 and sorted(ren.state_dict()) == sorted(ren._NAMES)
    assert sorted(sdf.sdf_layer.state_dict()) == sorted(sdf.sdf_layer._NAMES)
    assert list(var.state_dict()) == ["variance"]


def test_renderer_replicas_share_whole_image_state(fake):
    _, sdf, ren, var = make_networks(D)
    r = recon.SparseNeuSRenderer(None, sdf, var, ren, 64, 64, 0, 1.0, alpha_type="div")
    a, b = replicate_clones(r, 2)
    assert a._stats is r._stats and b._sides is r._sides
    assert a.sdf_network is not sdf and a.sdf_network.sdf_layer._packs is sdf.sdf_layer._packs
    before = recon.pack_stats()
    assert _bytes(a.sdf_network.sdf_layer.blob()) == _bytes(sdf.sdf_layer.blob()) and _bytes(b.rendering_network.x3_blob()) == _bytes(ren.x3_blob())
    assert sum(pack_delta(before).values()) == 2                              # one SDF blob, one pair of colour blobs: shared by source and replicas
    assert packs.param(a.variance_network, "variance") is a.variance_network.variance


def _mini_outputs(mod, sample):
    torch.manual_seed(0)
    return mod(sample, mode="export_mesh", resolution=20), mod(sample, mode="val")


def test_mini_trainer_replica_equals_the_source(fake):
    tr = MiniTrainer(D)
    sample, _ = make_sample(4, 24)
    want = _mini_outputs(tr, sample)
    assert want[0]["triangles"].shape[0] > 0
    for rnd in range(2):
        before = recon.pack_stats()
        rep = replicate_clones(tr, 2)[0]
        st0 = rep.sdf_renderer_lod0.whole_image_stats()
        got = _mini_outputs(rep, sample)
        st1 = tr.sdf_renderer_lod0.whole_image_stats()          # shared with the source: the replica's image was rendered whole
        assert st1["images"] == st0["images"] + 1 and st1["plain_calls"] == st0["plain_calls"], st1
        for w, g in zip(want, got):
            for k in w:
                assert torch.equal(w[k], g[k]), (rnd, k)
        assert pack_delta(before) == {}, "the source's packings serve the replicas on its device"


@pytest.mark.reference
def test_reference_trainer_on_a_replica(monkeypatch, tmp_path):
    from oracle import ref_import as RI
    if not RI.available():
        pytest.skip("/root/reference not present")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    with reference_trainer(monkeypatch, tmp_path) as (GenericTrainer, M):
        tr = build_reference_trainer(GenericTrainer, M, D)
        sample, _ = make_sample(4, 24)
        path = os.path.join(M.tmp, "mesh.ply")
        runs = []
        for which in ("source", "replica", "replica"):
            mod = tr if which == "source" else replicate_clones(tr, 2)[0]
            before = recon.pack_stats()
            if os.path.exists(path):
                os.remove(path)
            mod.export_mesh_step(sample, iter_step=0, chunk_size=512, resolution=20)
            mesh = mesh_io.read_ply(path)
            vm = types.MethodType(type(mod).validate_mesh, mod)
            mod.validate_mesh = lambda *a, _vm=vm, **k: _vm(*a, **dict(k, resolution=12))
            del M.written[:]
            torch.manual_seed(11)
            mod.val_step(sample, background_rgb=None, alpha_inter_ratio_lod0=1.0, iter_step=0, chunk_size=512, save_vis=True)
            images = sorted((os.path.relpath(p, M.tmp), img.tobytes()) for p, img in M.written)
            runs.append((mesh, images, torch.get_rng_state(), pack_delta(before)))
        (m0, i0, s0, _), rest = runs[0], runs[1:]
        assert m0[0].shape[0] > 0 and len(i0) == 3
        for m, i, s, d in rest:
            assert all(np.array_equal(a, b) for a, b in zip(m0, m) if a is not None) and (m0[2] is None) == (m[2] is None)
            assert i == i0 and torch.equal(s, s0)
            assert d == {}, d                                 # the replicas on the source's device: nothing re-packed
