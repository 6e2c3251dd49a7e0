"""The ray sampler's stage entries (csrc/render.hip), each alone, in both kernel forms, against the float64 references of tests/sampler_ref.py on the
seeded inputs that tests/test_sampler_ref_cpu.py has checked on the CPU (against the oracle, against the host build of csrc/render_math.h, and for
the caps of the tolerance rules).

Forms: O2345_RAY_STREAM_MIN = 0 (one lane per ray: k_ray_stream, k_ray_composite) and 10^9 (sixteen lanes per ray: k_ray_group,
k_ray_composite_group); up-sampling also with streaming=False (no scratch rows: the sixteen-lane kernel whatever the knob says).

Shapes: R in {1, 3, 5, 63, 65, 257} (a ragged group of four rays, a ragged wave, a second 256-thread block) and S in {2, 3, 9, 15, 16, 17, 64, 129, 255}
(around the blocks of 8 rows and the 16 lanes), each once per stage with R * S small; the per-stage sizes are listed in tests/sampler_ref.py.

Tolerances:
  rule E (element-wise values)  max |gpu - ref64| <= 4 e_ref + 4 ulp of the output's magnitude, e_ref = max |ref32 - ref64| of the same case
  rule Z (new depths)           per sample C * sens + 4 ulp(z) against the float64 inverse CDF of the KERNEL'S OWN section weights; sens = max over
                                the landed bin and its two neighbours of width / pdf mass, C = 4 x the normalised deviation of the float32 inverse
                                CDF on those weights; the bin's width for a sample whose bin mass is within 1e-3 of sample_pdf's 1e-5 switch
  exact                         depths without jitter, the merge, occupancy, lists and counts, defaults, colour mask, grad_err[:, 1]; form against form
Every comparison prints e_ref / C and the observed device error.

Observed on an MI355X, maxima over the cases (error, and its share of the bound; DESIGN.md section 4, "sampler stages: what pins what"):
  coarse      z 1.6e-7 (0.20), with jitter 3.2e-7 (0.08); points 2.3e-7 (0.22)
  weights     e_ref <= 8.9e-7, device 8.9e-7 (0.23)
  new depths  C <= 8.2e-6 (S = 255: 0.13 x 4 S 2^-24); device <= 0.25 of the bound in every case
  finalize    dists 1.2e-7 (0.96: one rounding), mid_z 1.2e-7 (0.77), points 2.4e-7 (0.59)
  composite   weights 1.4e-7 (0.25), cdf 1.4e-7 (0.14), colour 1.1e-6 (0.33), depth 2.4e-6 (0.29), weights_sum 1.5e-6 (0.26), depth_var 2.9e-10 (0.24),
              alpha_sum 2.0e-5 at a magnitude of 51 (0.57), grad_err[:, 0] 2.9e-5 at 131 (0.25)
With n_imp = 1 both forms returned NaN depths before linspace_at handled a single step (csrc/render_math.h)."""
import importlib

import pytest
import torch

import sampler_ref as SR

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FORMS = (("stream", "0"), ("group", "1000000000"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


def use_form(lib_instance, thr):
    assert ("ray_stream_min=" + thr).encode() in lib_instance({"O2345_RAY_STREAM_MIN": thr}).o2345_knobs()


def rm(t):
    """device SAMPLE-MAJOR [S,R,...] -> host ray-major [R,S,...]"""
    return t.detach().cpu().transpose(0, 1).contiguous()


def maskvol(dev):
    return SR.synthetic_mask().reshape(-1).contiguous().to(dev)


def check_e(got, ref32, ref64, what):
    e_ref, bound = SR.rule_e_bound(ref32, ref64)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{what}: e_ref {e_ref:.2e}, device err {err:.2e}, bound {bound:.2e}")
    assert err <= bound, f"{what}: device err {err:.3e} > 4 * {e_ref:.3e} + 4 ulp = {bound:.3e}"
    return err


# ------------------------------------------------------------------------------------------------ coarse samples
@pytest.mark.parametrize("R,S,variant", SR.COARSE_CASES)
def test_coarse(dev, ops, R, S, variant):
    d = SR.coarse_inputs(R, S, variant)
    on = lambda t: t.to(dev) if torch.is_tensor(t) else t
    z, pts = ops.ray_coarse(on(d["rays_o"]), on(d["rays_d"]), on(d["near"]), on(d["far"]), S, on(d["t_rand"]))
    z, pts = rm(z), rm(pts)
    z64, p64 = SR.coarse(d["rays_o"], d["rays_d"], d["near"], d["far"], S, d["t_rand"])
    if d["t_rand"] is None:                       # include/o2345.h: the oracle's float32 near + (far - near) * torch.linspace(0, 1, S), bit for bit
        assert torch.equal(z, SR.coarse(d["rays_o"], d["rays_d"], d["near"], d["far"], S, dtype=F32)[0])
    bz, bp = SR.coarse_bounds(d, z64, p64)
    ez, ep = (z.double() - z64).abs(), (pts.double() - p64).abs()
    print(f"coarse R={R} S={S} {variant} jitter={d['t_rand'] is not None}: z err {float(ez.max()):.2e} (bound {float(bz.max()):.2e}), "
          f"pts err {float(ep.max()):.2e} (bound {float(bp.max()):.2e})")
    assert bool((ez <= bz).all()) and bool((ep <= bp).all())


# ------------------------------------------------------------------------------------------------ up-sampling
@pytest.mark.parametrize("R,S,inv_s", SR.UPSAMPLE_CASES)
def test_upsample_weights(dev, ops, lib_instance, R, S, inv_s):
    """the streaming kernel's section weights alpha * T + 1e-5 (its scratch rows) against float64, rule E"""
    d = SR.upsample_inputs(R, S, inv_s)
    use_form(lib_instance, "0")
    out = ops.ray_upsample(d["rays_o"].to(dev), d["rays_d"].to(dev), SR.sm(d["z"]).to(dev), SR.sm(d["sdf"]).to(dev), inv_s, maskvol(dev), SR.MASK_D, 16,
                           want_weights=True)
    w32, w64 = (SR.upsample_weights(d["z"], d["sdf"], d["m"], inv_s, t) for t in (F32, F64))
    check_e(rm(out[3]), w32, w64, f"upsample weights R={R} S={S} inv_s={inv_s:g}")


def _upsample_all_forms(dev, ops, lib_instance, d, n_imp):
    a = (d["rays_o"].to(dev), d["rays_d"].to(dev), SR.sm(d["z"]).to(dev), SR.sm(d["sdf"]).to(dev), d["inv_s"], maskvol(dev), SR.MASK_D, n_imp)
    use_form(lib_instance, "0")
    stream = ops.ray_upsample(*a, want_weights=True)
    no_scratch = ops.ray_upsample(*a, streaming=False)
    use_form(lib_instance, "1000000000")
    group = ops.ray_upsample(*a)
    return stream, group, no_scratch


@pytest.mark.parametrize("n_imp", SR.UPSAMPLE_NIMP)
@pytest.mark.parametrize("R,S,inv_s", SR.UPSAMPLE_CASES)
def test_upsample_new_depths(dev, ops, lib_instance, R, S, inv_s, n_imp):
    d = SR.upsample_inputs(R, S, inv_s)
    stream, group, no_scratch = _upsample_all_forms(dev, ops, lib_instance, d, n_imp)
    for name, other in (("group", group), ("no scratch", no_scratch)):              # the forms: bit-identical, the lists as sets
        assert torch.equal(stream[0], other[0]) and torch.equal(stream[1], other[1]), name
        assert torch.equal(torch.sort(stream[2]).values, torch.sort(other[2]).values), name
    new_z, new_pts, lst = rm(stream[0]), rm(stream[1]), stream[2].cpu().long()
    assert torch.isfinite(new_z).all()
    z = d["z"]
    assert bool((new_z[:, 1:] >= new_z[:, :-1]).all()) and bool((new_z >= z[:, :1]).all()) and bool((new_z <= z[:, -1:]).all())
    # the points of the returned depths (two roundings per component), the list: their nearest-voxel occupancy, at most one entry reported as none
    p64, bp = SR.point_bound(d["rays_o"], d["rays_d"], new_z)
    assert bool(((new_pts.double() - p64).abs() <= bp).all())
    occ = SR.occupancy(SR.synthetic_mask(), new_pts) > 0                             # [R,n_imp]
    want = torch.nonzero(occ.T.reshape(-1)).flatten()                                # slots t * R + r
    if want.numel() <= 1:
        want = want[:0]
    assert torch.equal(torch.sort(lst).values, want)
    # rule Z on the kernel's own section weights
    fine = SR.fine_rays(d)
    if not bool(fine.any()) or (S, n_imp) in SR.RULE_Z_DROPPED:
        return
    q = SR.rule_z(z, rm(stream[3]))(n_imp)
    C = 4 * float(q["dev32"][fine].max())
    bound = SR.rule_z_bound(q, C, fine)
    err = (new_z.double() - q["new_z"]).abs()
    print(f"upsample depths R={R} S={S} inv_s={inv_s:g} n_imp={n_imp}: C {C:.2e} ({C / 4 / (S * 2.0 ** -24):.2f} x 4 S 2^-24), device err / bound "
          f"{float((err / bound)[fine].max()):.2f}, max err {float(err[fine].max()):.2e}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("R,S,n_new", SR.MERGE_CASES)
def test_merge(dev, ops, lib_instance, R, S, n_new):
    """cat_z_vals' merge, bit for bit the stable sort: n_new = 16 is the fused rank merge of either form, every other size k_ray_merge_any (blocks of 32)"""
    d = SR.merge_inputs(R, S, n_new)
    zz, ss = SR.merge(d["z"], d["sdf"], d["new_z"], d["new_sdf"])
    for name, thr in FORMS:
        use_form(lib_instance, thr)
        gz, gs = ops.ray_merge(SR.sm(d["z"]).to(dev), SR.sm(d["sdf"]).to(dev), SR.sm(d["new_z"]).to(dev), SR.sm(d["new_sdf"]).to(dev))
        bad = torch.nonzero((rm(gz) != zz).any(1) | (rm(gs) != ss).any(1)).flatten()
        assert bad.numel() == 0, (name, [(int(r), SR.MERGE_CONTENT[int(d["content"][r])]) for r in bad[:8]])


# ------------------------------------------------------------------------------------------------ finalize
@pytest.mark.parametrize("R,S", SR.FINALIZE_CASES)
def test_finalize(dev, ops, lib_instance, R, S):
    d = SR.finalize_inputs(R, S)
    mask = SR.synthetic_mask()
    f32_, f64_ = (SR.finalize(d["rays_o"], d["rays_d"], d["z"], d["sample_dist"], mask, dtype=t) for t in (F32, F64))
    bounds = SR.finalize_bounds(d, f64_)
    outs = {}
    for name, thr in FORMS:
        use_form(lib_instance, thr)
        o = outs[name] = ops.ray_finalize(d["rays_o"].to(dev), d["rays_d"].to(dev), SR.sm(d["z"]).to(dev), d["sample_dist"], maskvol(dev), SR.MASK_D)
        pm = rm(o["pm"])
        assert torch.equal(pm, f32_["pm"]) and torch.equal(pm, SR.occupancy(mask, rm(o["pts"])))          # exact
        assert bool((o["sdf"] == 100.0).all()) and bool((o["grad"] == 0).all()) and bool((o["rgb"] == 0).all())      # the defaults in every slot
        n = int(o["count"])
        want = torch.nonzero(pm.T.reshape(-1) > 0).flatten()                         # slots s * R + r
        assert n == want.numel() and torch.equal(torch.sort(o["list"][:n].cpu().long()).values, want)
        for k, b in bounds.items():
            e = (rm(o[k]).double() - f64_[k]).abs()
            print(f"finalize {name} R={R} S={S} {k}: device err {float(e.max()):.2e} (bound {float(b.max()):.2e})")
            assert bool((e <= b).all()), (name, k)
        assert bool((rm(o["dists"])[:, -1] == torch.tensor(d["sample_dist"], dtype=F32)).all())
    for k in ("mid_z", "dists", "pts", "pm"):
        assert torch.equal(outs["stream"][k], outs["group"][k]), k


# ------------------------------------------------------------------------------------------------ composite
@pytest.mark.parametrize("R,S,air,inv_s,bg", SR.COMPOSITE_CASES)
def test_composite(dev, ops, lib_instance, R, S, air, inv_s, bg):
    d = SR.composite_inputs(R, S, air, inv_s, bg)
    r32, r64 = SR.composite_refs(d)
    a = [d["rays_o"].to(dev), d["rays_d"].to(dev)] + [SR.sm(d[k]).to(dev) for k in ("mid_z", "dists", "pm", "sdf", "grad", "rgb", "nviews")]
    outs = {}
    for name, thr in FORMS:
        use_form(lib_instance, thr)
        outs[name] = ops.ray_composite(*a, inv_s, air, bg)
    for k in SR.COMPOSITE_OUTPUTS:                                                  # form against form, bit for bit
        assert torch.equal(outs["stream"][k], outs["group"][k]), k
    o = {k: (rm(v) if k in ("weights", "cdf") else v.cpu()) for k, v in outs["stream"].items()}
    assert torch.equal(o["color_mask"].bool(), r64["color_mask"])                    # exact
    assert torch.equal(o["grad_err"][:, 1].double(), r64["grad_err"][:, 1])
    for k in SR.COMPOSITE_OUTPUTS[:-1]:                                             # rule E
        pick = (lambda t: t[:, 0]) if k == "grad_err" else (lambda t: t)
        check_e(pick(o[k]), pick(r32[k]), pick(r64[k]), f"composite R={R} S={S} ratio={air:g} inv_s={inv_s:g} bg={bg:g} {k}")
