"""nn.DataParallel replicas of the mirror modules on the MI355X.

* Two replicas on ONE device (torch's replicate() with the broadcast patched to same-device clones, tests/dp_util.py), run by two host threads with a
  stream each -- what DataParallel's parallel_apply does with one device per thread -- on two different seeded scenes: every replica's mesh (vertices,
  triangles, vertex colours) and 256 x 256 val image is bit-identical to the sequential, un-replicated result of its scene, and the second round
  packs nothing (recon.pack_stats()).
* A real nn.DataParallel(device_ids=[0, 1]) over a batch of two scenes (skipped with fewer than two devices): the same checks, every device packed and
  preloaded once."""
import threading
import time

import pytest
import torch

from dp_util import MiniTrainer, batch_samples, make_sample, pack_delta, recon, replicate_clones

pytestmark = pytest.mark.gpu
D, HW, RES = 32, 256, 64
SEEDS = (5, 9)


def _run(mod, sample):
    torch.manual_seed(0)
    return {"export_mesh": mod(sample, mode="export_mesh", resolution=RES), "val": mod(sample, mode="val")}


def _same(want, got):
    for mode in ("export_mesh", "val"):
        for k, w in want[mode].items():
            g = got[mode][k].cpu()
            assert w.shape == g.shape and torch.equal(w.cpu(), g), (mode, k)


@pytest.fixture(scope="module")
def scenes():
    dev = torch.device("cuda:0")
    samples = [make_sample(4, HW, seed=s, device=dev, batch_idx=i)[0] for i, s in enumerate(SEEDS)]
    base = MiniTrainer(D).to(dev)                             # the sequential, un-replicated results (its own pack caches)
    want = [_run(base, s) for s in samples]
    assert all(w["export_mesh"]["triangles"].shape[0] > 0 for w in want)
    return dev, samples, want


def test_two_replicas_on_one_device_two_threads(scenes):
    dev, samples, want = scenes
    tr = MiniTrainer(D).to(dev)                               # identically seeded, nothing packed yet
    times, deltas = [], []
    for rnd in range(2):
        before = recon.pack_stats()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        reps = replicate_clones(tr, 2)
        got, errs = [None, None], []

        def work(i):
            try:
                s = torch.cuda.Stream(dev)
                with torch.cuda.device(dev), torch.cuda.stream(s):
                    got[i] = _run(reps[i], samples[i])
                    s.synchronize()
            except BaseException as e:                    # noqa: BLE001 -- re-raised in the main thread
                errs.append(e)
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        times.append(time.perf_counter() - t0)
        if errs:
            raise errs[0]
        deltas.append(pack_delta(before))
        for i in range(2):
            _same(want[i], got[i])
    print(f"\nreplicated round on one device (two threads, two scenes): first {1e3 * times[0]:.1f} ms (packs {deltas[0]}), "
          f"second {1e3 * times[1]:.1f} ms (packs {deltas[1]})")
    assert deltas[0] and all(v == (12 if k[0] == "conv" else 1) for k, v in deltas[0].items() if k[0] != "sdf_grid"), deltas[0]
    assert deltas[1] == {}, "the second round re-packed"


def test_one_replica_serves_whole_images(scenes):
    """A single-scene forward under DataParallel with >= 2 devices replicates onto device_ids[0] and runs it in the calling thread: whole images."""
    dev, samples, want = scenes
    tr = MiniTrainer(D).to(dev)
    rep = replicate_clones(tr, 1)[0]
    st0 = rep.sdf_renderer_lod0.whole_image_stats()
    _same(want[0], _run(rep, samples[0]))
    st1 = tr.sdf_renderer_lod0.whole_image_stats()               # the counters are shared with the source
    assert st1["images"] == st0["images"] + 1 and st1["plain_calls"] == st0["plain_calls"], st1


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_dataparallel_over_two_devices(scenes):
    dev, samples, want = scenes
    sink = {}
    tr = MiniTrainer(D, sink=sink).to(dev)
    dp = torch.nn.DataParallel(tr, device_ids=[0, 1])
    batch = batch_samples(samples)
    times, deltas = [], []
    for rnd in range(2):
        before = recon.pack_stats()
        t0 = time.perf_counter()
        for mode, kw in (("export_mesh", dict(resolution=RES)), ("val", {})):
            torch.manual_seed(0)
            dp(batch, mode=mode, **kw)
        for d in (0, 1):
            torch.cuda.synchronize(d)
        times.append(time.perf_counter() - t0)
        deltas.append(pack_delta(before))
        for i in range(2):
            _same(want[i], {m: sink[(i, m)] for m in ("export_mesh", "val")})
    print(f"\nnn.DataParallel over cuda:0, cuda:1 (two scenes): first round {1e3 * times[0]:.1f} ms (packs {deltas[0]}), "
          f"second {1e3 * times[1]:.1f} ms (packs {deltas[1]})")
    assert {k[1] for k in deltas[0]} == {"cuda:0", "cuda:1"} and all(v == (12 if k[0] == "conv" else 1) for k, v in deltas[0].items()
                                                                     if k[0] != "sdf_grid"), deltas[0]
    assert deltas[1] == {}
    st = recon.pack_stats()
    assert st.get(("preload", "cuda:0")) == 1 and st.get(("preload", "cuda:1")) == 1
