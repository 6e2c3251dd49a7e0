"""Numerical mode of the network kernels.

``PRECISION`` (environment ``O2345_PRECISION``) selects how the dense layers of the SDF and colour networks are evaluated:

* ``"f16x3"`` (default)  every fp32 operand is split into two f16 halves (hi + lo, 22 significant bits) and each product is
  accumulated in fp32 as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16.  fp32-class accuracy (measured deviation from the
  oracle within 1.5x of the exact fp32 MFMA chain's), 5.3x less matrix time than the fp32 MFMA.
* ``"fp32"``  v_mfma_f32_32x32x2_f32, the exact fp32 FMA chain (strict mode).

(Rounds 1-2 also had a ``"bf16"`` SDF mode for BASELINE config 2's "bf16 SDF MLP" wording.  It was 1000x less accurate than the default and, since the
register fix of the default gradient kernel in round 3, slower as well (10.9 vs 9.9 ms): removed.)

The convolutions (FeatureNet, compress layer, sparse cost-regularisation network) follow the COLOUR mode: split-f16 on the matrix cores by
default, fp32 VALU kernels in ``"fp32"`` mode -- per object when a mode is handed to ``pipeline.SceneWeights`` / ``featurenet.set_precision``,
else this global one.  Cost-volume gather, sampling, compositing and marching cubes are precision-independent (fp32 / fp64 / integer)."""
import os
from collections import namedtuple

PRECISIONS = ("f16x3", "fp32")
PRECISION = os.environ.get("O2345_PRECISION", "f16x3")
if PRECISION not in PRECISIONS:
    raise ValueError(f"O2345_PRECISION must be one of {PRECISIONS}, got {PRECISION!r}")


def sdf_precision(p=None):
    p = PRECISION if p is None else p
    if p not in PRECISIONS:
        raise ValueError(f"unknown precision {p!r}")
    return p


def color_precision(p=None):
    p = PRECISION if p is None else p
    if p not in PRECISIONS:
        raise ValueError(f"unknown precision {p!r}")
    return p


# ---- tolerance-bounded colour work removal (include/o2345.h, O2345RenderIO.weight_cull) ----------------------------------------
# render(): the colour network (59 % of a render call) is evaluated only on occupied samples whose compositing weight w = alpha * T -- known after the
# SDF + gradient pass, before any colour -- is >= WEIGHT_CULL.  Colours lie in [0, 1], so a ray's colour moves by at most 128 * 2^-24 = 7.6e-6, a quarter
# of the 3e-5 stage tolerance; depth, weights, gradients and the colour mask are untouched.  What qualifies are the samples BEHIND a surface (T ~ 0):
# 6 % of the occupied samples at the untrained variance 0.2 (inv_s 7.4), 27 % / 47 % at a trained model's 0.45 / 0.65 (bench.py, `trained_regime`);
# free-space samples keep the reference's +1e-5 (w ~ 1e-5) and are never dropped.  O2345_WEIGHT_CULL=0 selects the exhaustive path (every occupied
# sample, the reference's work); both are tested.
# The bound assumes blended colours in [0, 1] (the reference's colour maps are images in [0, 1], One2345_eval_new_data.py:199-201; the blend is a convex
# combination of them): for maps of another range the bound scales with that range -- set O2345_WEIGHT_CULL accordingly.  "" or "0" = off, like the other knobs.
WEIGHT_CULL = float(os.environ.get("O2345_WEIGHT_CULL", "").strip() or 0.0) if "O2345_WEIGHT_CULL" in os.environ else 2.0 ** -24
if not (0.0 <= WEIGHT_CULL < 1.0):
    raise ValueError(f"O2345_WEIGHT_CULL must be in [0, 1), got {WEIGHT_CULL}")


def weight_cull(w=None):
    w = WEIGHT_CULL if w is None else float(w)
    if not (0.0 <= w < 1.0):
        raise ValueError(f"weight_cull must be in [0, 1), got {w}")
    return w


def warm_aten():
    """O2345_WARM_ATEN (default on): ops.preload() also launches, once on tiny tensors, the few ATen kernels the unchanged trainer runs inside its own timing
    brackets, so that their first-launch cost in a fresh process (2 - 14 ms each) is paid when the weights are loaded."""
    return os.environ.get("O2345_WARM_ATEN", "1") not in ("", "0")


def prepack_resolutions():
    """O2345_PREPACK_RESOLUTIONS (default "256" = run.py's --resolution, run.py:61-67): extraction-lattice resolutions whose layer-0 tables are built when the
    weights are loaded (2 ms each) instead of inside the first extract_fields call; any other resolution is built on first use."""
    v = os.environ.get("O2345_PREPACK_RESOLUTIONS", "256")
    return tuple(int(x) for x in v.replace(",", " ").split())


def _non_negative_int(name, text):
    t = text.strip()
    if t == "":
        return 0
    if not t.isdigit():
        raise ValueError(f"{name} must be a non-negative integer, got {text!r}")
    return int(t)


# ---- background table of the extraction lattice (csrc/sdf_mlp_x3.hip, o2345_sdf_grid_sparse_x3) ---------------------------------------------------------
# A lattice point without a kept voxel among its trilinear corners has the SDF of an empty scene, which depends on the weights and the resolution only:
# pipeline.SceneWeights.grid_background keeps that field, R^3 floats per (weights, R), from the SECOND extraction at a resolution on, and the lattice
# kernel then runs on the tiles that touch the scene only.  O2345_GRID_BACKGROUND_MB is the largest table kept, in MiB: unset or "" = 256 (R <= 406),
# 0 = never (every extraction evaluates the whole lattice, as before); a table over the budget or R^3 >= 2^31 means the same.  Results are identical.
_gb = os.environ.get("O2345_GRID_BACKGROUND_MB", "")
GRID_BACKGROUND_MB = 256 if _gb.strip() == "" else _non_negative_int("O2345_GRID_BACKGROUND_MB", _gb)
del _gb


def grid_background_mb():
    return GRID_BACKGROUND_MB


def grid_background_allowed(resolution):
    """True when a background table for this resolution fits the budget and the sparse evaluation's 32-bit slots."""
    n = int(resolution) ** 3
    return n < 2 ** 31 and 4 * n <= grid_background_mb() << 20


# ---- mesh component filter (csrc/mesh_components.hip; mesh_io.filter_components is the host twin) ----------------------------------------------------
# O2345_MESH_MIN_COMPONENT_FACES=n drops the connected components of the extracted mesh with fewer than n faces; O2345_MESH_KEEP_LARGEST=1 keeps only the
# component with the most faces (ties: the smaller label), among what the threshold left.  Both off by default ("" or "0" = off, like the other knobs): the
# mesh is then what marching cubes found, as before.  The filter runs on the device between marching cubes and vertex colouring.
MESH_MIN_COMPONENT_FACES = _non_negative_int("O2345_MESH_MIN_COMPONENT_FACES", os.environ.get("O2345_MESH_MIN_COMPONENT_FACES", ""))
MESH_KEEP_LARGEST = _non_negative_int("O2345_MESH_KEEP_LARGEST", os.environ.get("O2345_MESH_KEEP_LARGEST", "")) != 0


def mesh_min_component_faces(n=None):
    """None -> the configured default; anything else must be a non-negative integer."""
    if n is None:
        return MESH_MIN_COMPONENT_FACES
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"min_component_faces must be a non-negative integer, got {n!r}")
    return int(n)


def mesh_keep_largest(k=None):
    return MESH_KEEP_LARGEST if k is None else bool(k)


# ---- mesh smoothing (csrc/mesh_smooth.hip; mesh_io.smooth_vertices is the host twin) -------------------------------------------------------------------
# O2345_MESH_SMOOTH_ITERATIONS=n runs n iterations of Taubin's lambda|mu filter on the extracted mesh's vertex positions, on the device, after the vertex
# colours were taken at the unsmoothed vertices ("" or "0" = off, the default: the mesh is then what marching cubes found, and nothing is launched).
# O2345_MESH_SMOOTH_LAMBDA (0.5, in (0, 1]) and O2345_MESH_SMOOTH_MU (-0.53, <= 0; 0 = plain Laplacian smoothing, which shrinks the shape) are the two
# factors of one iteration; O2345_MESH_SMOOTH_PIN_BOUNDARY (1) keeps the vertices on open edges (the rim of a mesh cut by the volume's faces) in place.
def _finite_float(name, text, default, ok, what):
    t = text.strip()
    if t == "":
        return default
    try:
        x = float(t)
    except ValueError:
        x = float("nan")
    if not (x == x and abs(x) != float("inf") and ok(x)):
        raise ValueError(f"{name} must be {what}, got {text!r}")
    return x


MESH_SMOOTH_ITERATIONS = _non_negative_int("O2345_MESH_SMOOTH_ITERATIONS", os.environ.get("O2345_MESH_SMOOTH_ITERATIONS", ""))
MESH_SMOOTH_LAMBDA = _finite_float("O2345_MESH_SMOOTH_LAMBDA", os.environ.get("O2345_MESH_SMOOTH_LAMBDA", ""), 0.5, lambda x: 0.0 < x <= 1.0, "in (0, 1]")
MESH_SMOOTH_MU = _finite_float("O2345_MESH_SMOOTH_MU", os.environ.get("O2345_MESH_SMOOTH_MU", ""), -0.53, lambda x: x <= 0.0, "finite and <= 0")
_pin = os.environ.get("O2345_MESH_SMOOTH_PIN_BOUNDARY", "")
MESH_SMOOTH_PIN_BOUNDARY = True if _pin.strip() == "" else _non_negative_int("O2345_MESH_SMOOTH_PIN_BOUNDARY", _pin) != 0
del _pin


def mesh_smooth_iterations(n=None):
    """None -> the configured default; anything else must be a non-negative integer."""
    if n is None:
        return MESH_SMOOTH_ITERATIONS
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"smooth_iterations must be a non-negative integer, got {n!r}")
    return int(n)


def mesh_smooth_lambda(lam=None):
    if lam is None:
        return MESH_SMOOTH_LAMBDA
    return _finite_float("lam", repr(float(lam)), None, lambda x: 0.0 < x <= 1.0, "in (0, 1]")


def mesh_smooth_mu(mu=None):
    if mu is None:
        return MESH_SMOOTH_MU
    return _finite_float("mu", repr(float(mu)), None, lambda x: x <= 0.0, "finite and <= 0")


def mesh_smooth_pin_boundary(p=None):
    return MESH_SMOOTH_PIN_BOUNDARY if p is None else bool(p)


# ---- mesh decimation (csrc/mesh_decimate.hip; mesh_io.decimate_mesh is the host twin) -------------------------------------------------------------------
# O2345_MESH_DECIMATE_CELL=c merges the vertices of the extracted mesh that share a lattice cell of edge c (in units of the extraction grid's spacing) into
# one vertex at their mean and drops the triangles that collapse, on the device, after the component filter and before the vertices are coloured ("" or
# "0" = off, the default: the mesh is then what marching cubes found, and nothing is launched).
MESH_DECIMATE_CELL = _finite_float("O2345_MESH_DECIMATE_CELL", os.environ.get("O2345_MESH_DECIMATE_CELL", ""), 0.0, lambda x: x >= 0.0, "a finite float >= 0")


def mesh_decimate_cell(x=None):
    """None -> the configured default; anything else must be a finite float >= 0 (an explicit 0 is off whatever the default)."""
    if x is None:
        return MESH_DECIMATE_CELL
    return _finite_float("decimate_cell", repr(float(x)), None, lambda c: c >= 0.0, "a finite float >= 0")


# ---- mesh simplification (csrc/mesh_simplify.hip; mesh_io.simplify_mesh is the host twin) ---------------------------------------------------------------
# O2345_MESH_SIMPLIFY_FACES=n simplifies the extracted mesh to at most n triangles, if reachable, by rounds of half-edge collapses ordered by quadric
# error, on the device, after the decimation and before the projection ("" or "0" = off, the default: nothing is launched).  O2345_MESH_SIMPLIFY_MAX_ERROR
# ("" = no limit) is the largest quadric error of a collapse, in squared grid spacings times area; O2345_MESH_SIMPLIFY_MAX_ROUNDS (256) the number of rounds.
def _max_error(name, text):
    t = text.strip()
    try:
        x = float("inf") if t == "" else float(t)
    except ValueError:
        x = float("nan")
    if not x >= 0.0:
        raise ValueError(f"{name} must be a float >= 0 (inf = no limit), got {text!r}")
    return x


def _below_2_31(name, n):
    if n >= 2 ** 31:
        raise ValueError(f"{name} must be a non-negative integer below 2^31, got {n!r}")
    return n


MESH_SIMPLIFY_FACES = _below_2_31("O2345_MESH_SIMPLIFY_FACES", _non_negative_int("O2345_MESH_SIMPLIFY_FACES", os.environ.get("O2345_MESH_SIMPLIFY_FACES", "")))
MESH_SIMPLIFY_MAX_ERROR = _max_error("O2345_MESH_SIMPLIFY_MAX_ERROR", os.environ.get("O2345_MESH_SIMPLIFY_MAX_ERROR", ""))
_rounds = os.environ.get("O2345_MESH_SIMPLIFY_MAX_ROUNDS", "")
MESH_SIMPLIFY_MAX_ROUNDS = 256 if _rounds.strip() == "" else _below_2_31("O2345_MESH_SIMPLIFY_MAX_ROUNDS", _non_negative_int("O2345_MESH_SIMPLIFY_MAX_ROUNDS", _rounds))
del _rounds


def mesh_simplify_faces(n=None):
    """None -> the configured default; anything else must be a non-negative integer below 2^31 (an explicit 0 is off whatever the default)."""
    if n is None:
        return MESH_SIMPLIFY_FACES
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"simplify_faces must be a non-negative integer below 2^31, got {n!r}")
    return _below_2_31("simplify_faces", int(n))


def mesh_simplify_max_error(x=None):
    """None -> the configured default (inf: no limit); anything else must be a float >= 0."""
    return MESH_SIMPLIFY_MAX_ERROR if x is None else _max_error("max_error", repr(float(x)))


def mesh_simplify_max_rounds(n=None):
    if n is None:
        return MESH_SIMPLIFY_MAX_ROUNDS
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"max_rounds must be a non-negative integer below 2^31, got {n!r}")
    return _below_2_31("max_rounds", int(n))


# ---- mesh projection (csrc/mesh_project.hip; mesh_io.project_vertices is the host twin) -----------------------------------------------------------------
# O2345_MESH_PROJECT_ITERATIONS=n moves the vertices of the extracted mesh onto the SDF's zero set with up to n Newton steps p <- p - s g / |g|^2 on the
# device, after the decimation and before the vertices are coloured ("" or "0" = off, the default: nothing is launched; at most 64).
# O2345_MESH_PROJECT_TOL (5e-5: the SDF tolerance DESIGN.md section 4 states -- projecting further than the field is accurate is pointless) is the |sdf| at
# which a vertex counts as converged, O2345_MESH_PROJECT_MAX_STEP (0.5) the largest step per axis and round and O2345_MESH_PROJECT_MAX_MOVE ("" = max(1,
# decimate cell), so that a cluster mean can travel back as far as its cell allows) the half edge of the box around its start that a vertex never leaves,
# both in grid spacings.
def _project_iterations(name, n):
    if n > 64:
        raise ValueError(f"{name} must be an integer in [0, 64], got {n!r}")
    return n


MESH_PROJECT_ITERATIONS = _project_iterations("O2345_MESH_PROJECT_ITERATIONS",
                                              _non_negative_int("O2345_MESH_PROJECT_ITERATIONS", os.environ.get("O2345_MESH_PROJECT_ITERATIONS", "")))
MESH_PROJECT_TOL = _finite_float("O2345_MESH_PROJECT_TOL", os.environ.get("O2345_MESH_PROJECT_TOL", ""), 5e-5, lambda x: x >= 0.0, "a finite float >= 0")
MESH_PROJECT_MAX_STEP = _finite_float("O2345_MESH_PROJECT_MAX_STEP", os.environ.get("O2345_MESH_PROJECT_MAX_STEP", ""), 0.5, lambda x: x > 0.0, "a finite float > 0")
MESH_PROJECT_MAX_MOVE = _finite_float("O2345_MESH_PROJECT_MAX_MOVE", os.environ.get("O2345_MESH_PROJECT_MAX_MOVE", ""), None, lambda x: x > 0.0, "a finite float > 0")


def mesh_project_iterations(n=None):
    """None -> the configured default; anything else must be an integer in [0, 64] (an explicit 0 is off whatever the default)."""
    if n is None:
        return MESH_PROJECT_ITERATIONS
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"project_iterations must be an integer in [0, 64], got {n!r}")
    return _project_iterations("project_iterations", int(n))


def mesh_project_tol(x=None):
    if x is None:
        return MESH_PROJECT_TOL
    return _finite_float("tol", repr(float(x)), None, lambda t: t >= 0.0, "a finite float >= 0")


def mesh_project_max_step(x=None):
    if x is None:
        return MESH_PROJECT_MAX_STEP
    return _finite_float("max_step", repr(float(x)), None, lambda t: t > 0.0, "a finite float > 0")


def mesh_project_max_move(x=None, decimate_cell=None):
    """None -> the configured default, and where that is unset max(1, decimate cell) with the cell of this call (None: the configured one)."""
    if x is not None:
        return _finite_float("max_move", repr(float(x)), None, lambda t: t > 0.0, "a finite float > 0")
    if MESH_PROJECT_MAX_MOVE is not None:
        return MESH_PROJECT_MAX_MOVE
    return max(1.0, mesh_decimate_cell(decimate_cell))


# ---- texture atlas (csrc/mesh_texture.hip; mesh_io.texture_points / pack_texture / texture_corners are the host twins) -------------------------------------
# O2345_MESH_TEXTURE_TEXEL=c bakes a texture atlas for the exported .glb / .obj asset on the device: every pair of triangles gets a square cell of c x c
# texels (an integer in [4, 64]), the colour network is evaluated at every texel's surface point, and the asset carries texture coordinates and a PNG
# instead of vertex colours ("" or "0" = off, the default: nothing is launched and every file keeps its bytes).  O2345_MESH_TEXTURE_PNG_LEVEL (1) is the
# zlib level of that PNG, 0 .. 9, 0 = stored: compression is host time and dominates the textured export.
def _texture_texel(name, n):
    if not (n == 0 or 4 <= n <= 64):
        raise ValueError(f"{name} must be 0 (off) or an integer in [4, 64], got {n!r}")
    return n


def _png_level(name, n):
    if n > 9:
        raise ValueError(f"{name} must be an integer in [0, 9], got {n!r}")
    return n


MESH_TEXTURE_TEXEL = _texture_texel("O2345_MESH_TEXTURE_TEXEL", _non_negative_int("O2345_MESH_TEXTURE_TEXEL", os.environ.get("O2345_MESH_TEXTURE_TEXEL", "")))
_lvl = os.environ.get("O2345_MESH_TEXTURE_PNG_LEVEL", "")
MESH_TEXTURE_PNG_LEVEL = 1 if _lvl.strip() == "" else _png_level("O2345_MESH_TEXTURE_PNG_LEVEL", _non_negative_int("O2345_MESH_TEXTURE_PNG_LEVEL", _lvl))
del _lvl


def mesh_texture_texel(n=None):
    """None -> the configured default; anything else must be 0 (off, whatever the default) or an integer in [4, 64]."""
    if n is None:
        return MESH_TEXTURE_TEXEL
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"texture_texel must be 0 (off) or an integer in [4, 64], got {n!r}")
    return _texture_texel("texture_texel", int(n))


# the options of the mesh path, resolved and validated (mesh_options; 0 / False = off); project_max_move: the projection's move limit for this decimate_cell
# simplify_faces is the last field and defaults to 0 (off), so that a record built from the seven older fields compares equal to one with the stage off
MeshOptions = namedtuple("MeshOptions", "min_component_faces keep_largest decimate_cell project_iterations project_max_move smooth_iterations texture_texel "
                         "simplify_faces", defaults=(0,))


def mesh_options(min_component_faces=None, keep_largest=None, decimate_cell=None, project_iterations=None, smooth_iterations=None, texture_texel=None,
                 simplify_faces=None):
    """Every option of the mesh path through its validator, once per call: None -> the module constant as it is NOW, anything else as given."""
    cell = mesh_decimate_cell(decimate_cell)
    return MeshOptions(mesh_min_component_faces(min_component_faces), mesh_keep_largest(keep_largest), cell, mesh_project_iterations(project_iterations),
                       mesh_project_max_move(None, cell), mesh_smooth_iterations(smooth_iterations), mesh_texture_texel(texture_texel),
                       mesh_simplify_faces(simplify_faces))


def mesh_texture_png_level(n=None):
    if n is None:
        return MESH_TEXTURE_PNG_LEVEL
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"png_level must be an integer in [0, 9], got {n!r}")
    return _png_level("png_level", int(n))


# ---- normal map of the textured asset (csrc/mesh_texture.hip; mesh_io.texture_frames / pack_normal_map are the host twins) ----------------------------------
# O2345_MESH_NORMAL_MAP=1 makes the textured export also bake a tangent-space normal map: the SDF gradient at every texel's surface point, which the colour
# network needed anyway, in the tangent frame of the texel's triangle; the .glb gains TANGENT and a second image, the .obj a stem_normal.png ("" or "0" =
# off, the default: nothing is launched and every file keeps its bytes).  It needs the texture atlas: with texture_texel off it is an error, not a no-op.
MESH_NORMAL_MAP = _non_negative_int("O2345_MESH_NORMAL_MAP", os.environ.get("O2345_MESH_NORMAL_MAP", "")) != 0


def mesh_normal_map(x=None):
    return MESH_NORMAL_MAP if x is None else bool(x)


# ---- ambient occlusion map (csrc/mesh_raycast.hip; mesh_io.mesh_occlusion is the host twin) ---------------------------------------------------------------
# O2345_MESH_OCCLUSION=1 makes the textured export also bake an ambient occlusion map: at every texel's point on the final mesh, the share of
# O2345_MESH_OCCLUSION_SAMPLES cosine-weighted rays about the face normal (on the side the SDF gradient points to) that reach
# O2345_MESH_OCCLUSION_DISTANCE index units without hitting the mesh; the .glb gains an occlusionTexture, the .obj a stem_occlusion.png ("" or "0" = off,
# the default: nothing is launched and every file keeps its bytes).  It needs the texture atlas: with texture_texel off it is an error, not a no-op.
# Samples: "" = 64, at most 1024.  Distance: "" = resolution / 8 index units (an eighth of the scene's box: contact shading, not sky visibility).  The rays
# start MESH_OCCLUSION_BIAS = 1e-3 index units off the surface.
MESH_OCCLUSION = _non_negative_int("O2345_MESH_OCCLUSION", os.environ.get("O2345_MESH_OCCLUSION", "")) != 0
MESH_OCCLUSION_SAMPLES = _non_negative_int("O2345_MESH_OCCLUSION_SAMPLES", os.environ.get("O2345_MESH_OCCLUSION_SAMPLES", "")) or 64
MESH_OCCLUSION_BIAS = 1e-3


def _occlusion_distance(name, text):
    if text.strip() == "":
        return 0.0
    try:
        d = float(text)
    except ValueError:
        d = -1.0
    if not (0.0 < d < float("inf")):
        raise ValueError(f"{name} must be a finite number > 0 (index units), got {text!r}")
    return d


MESH_OCCLUSION_DISTANCE = _occlusion_distance("O2345_MESH_OCCLUSION_DISTANCE", os.environ.get("O2345_MESH_OCCLUSION_DISTANCE", ""))
if not 1 <= MESH_OCCLUSION_SAMPLES <= 1024:
    raise ValueError(f"O2345_MESH_OCCLUSION_SAMPLES must be in 1 .. 1024, got {MESH_OCCLUSION_SAMPLES}")


def mesh_occlusion(x=None):
    return MESH_OCCLUSION if x is None else bool(x)


def mesh_occlusion_distance(resolution):
    """the length of an occlusion ray in index units of a ``resolution``^3 lattice"""
    return MESH_OCCLUSION_DISTANCE or resolution / 8.0


# ---- mesh error report (csrc/mesh_distance.hip; mesh_io.mesh_distance is the host twin) -------------------------------------------------------------------
# O2345_MESH_ERROR=1 makes pipeline.reconstruct_folder report how far the mesh it wrote is from the raw marching-cubes mesh it started from, as surfaces:
# Chamfer, Hausdorff and F-score (ops.mesh_distance) in units of the extraction grid's spacing ("" or "0" = off, the default: nothing is launched and the
# result keeps its keys).
MESH_ERROR = _non_negative_int("O2345_MESH_ERROR", os.environ.get("O2345_MESH_ERROR", "")) != 0


def mesh_error(x=None):
    return MESH_ERROR if x is None else bool(x)


# ---- mesh audit report (csrc/mesh_audit.hip; mesh_io.mesh_audit is the host twin) -------------------------------------------------------------------------
# O2345_MESH_AUDIT=1 makes pipeline.reconstruct_folder report whether the mesh it wrote is a closed, oriented 2-manifold and how good its triangles are
# (ops.mesh_audit: open, non-manifold and inconsistent edges, bow-tie vertices, Euler characteristic, genus, area, volume, quality), in units of the
# extraction grid's spacing ("" or "0" = off, the default: nothing is launched and the result keeps its keys).
MESH_AUDIT = _non_negative_int("O2345_MESH_AUDIT", os.environ.get("O2345_MESH_AUDIT", "")) != 0


def mesh_audit(x=None):
    return MESH_AUDIT if x is None else bool(x)


# ---- self-intersection report (csrc/mesh_intersect.hip; mesh_io.mesh_intersections is the host twin) -----------------------------------------------------
# O2345_MESH_INTERSECTIONS=1 makes pipeline.reconstruct_folder report how many pairs of triangles of the mesh it wrote cross each other
# (ops.mesh_intersections: candidates, pairs, faces hit, the most pairs on one face) -- what the audit, a statement about connectivity, cannot say ("" or
# "0" = off, the default: nothing is launched and the result keeps its keys).
MESH_INTERSECTIONS = _non_negative_int("O2345_MESH_INTERSECTIONS", os.environ.get("O2345_MESH_INTERSECTIONS", "")) != 0


def mesh_intersections(x=None):
    return MESH_INTERSECTIONS if x is None else bool(x)


# ---- hole filling (csrc/mesh_fill.hip; mesh_io.fill_holes is the host twin) -------------------------------------------------------------------------------
# O2345_MESH_FILL_HOLES=n closes the boundary loops of the extracted mesh that have at most n edges, on the device, directly after the clean-up chain and
# before the vertices are coloured: a loop of three edges gets one triangle, a longer one a fan around its centroid ("" or "0" = off, the default: nothing
# is launched and every file keeps its bytes; n >= 3; MESH_FILL_HOLES_ALL = every hole).  Not a field of MeshOptions: a keyword of its own.
MESH_FILL_HOLES_ALL = 2 ** 31 - 1


def _fill_holes(name, n):
    if n in (1, 2):
        raise ValueError(f"{name} must be 0 (off) or an integer >= 3 (a hole has at least three edges), got {n!r}")
    return _below_2_31(name, n)


MESH_FILL_HOLES = _fill_holes("O2345_MESH_FILL_HOLES", _non_negative_int("O2345_MESH_FILL_HOLES", os.environ.get("O2345_MESH_FILL_HOLES", "")))


def mesh_fill_holes(n=None):
    """None -> the configured default; anything else must be 0 (off, whatever the default) or an integer in [3, 2^31): the longest hole, in edges, that is
    filled."""
    if n is None:
        return MESH_FILL_HOLES
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"fill_holes must be 0 (off) or an integer >= 3 below 2^31, got {n!r}")
    return _fill_holes("fill_holes", int(n))


# ---- surface render (csrc/surface_trace.hip; surface.py is the host twin) ---------------------------------------------------------------------------------
# pipeline.render_surface marches rays through the extraction lattice.  O2345_SURFACE_STRIDE (1.0, in (0, 8]) is the distance between two samples in
# lattice spacings -- above 1 the march may step over parts thinner than the stride; O2345_SURFACE_REFINE (8, in [0, 32]) the number of bracket
# refinements per hit.  O2345_PREVIEW_VIEWS=n makes pipeline.reconstruct_folder write n preview images next to the mesh ("" or "0" = off, the default:
# nothing is launched and the result keeps its keys).
SURFACE_STRIDE = _finite_float("O2345_SURFACE_STRIDE", os.environ.get("O2345_SURFACE_STRIDE", ""), 1.0, lambda x: 0.0 < x <= 8.0, "in (0, 8]")
_ref = os.environ.get("O2345_SURFACE_REFINE", "")
SURFACE_REFINE = 8 if _ref.strip() == "" else _non_negative_int("O2345_SURFACE_REFINE", _ref)
del _ref
if SURFACE_REFINE > 32:
    raise ValueError(f"O2345_SURFACE_REFINE must be an integer in [0, 32], got {SURFACE_REFINE!r}")
PREVIEW_VIEWS = _non_negative_int("O2345_PREVIEW_VIEWS", os.environ.get("O2345_PREVIEW_VIEWS", ""))


def surface_stride(x=None):
    if x is None:
        return SURFACE_STRIDE
    return _finite_float("stride", repr(float(x)), None, lambda s: 0.0 < s <= 8.0, "in (0, 8]")


def surface_refine(n=None):
    if n is None:
        return SURFACE_REFINE
    if isinstance(n, bool) or int(n) != n or not 0 <= n <= 32:
        raise ValueError(f"refine must be an integer in [0, 32], got {n!r}")
    return int(n)


# O2345_MESH_PREVIEW_VIEWS=n makes pipeline.reconstruct_folder rasterize the FINAL mesh (after the clean-up chain and the hole filling; csrc/mesh_raster.hip,
# raster.py is the host twin) from the cameras of the surface previews and write mesh_preview_000.png ... next to the PLY ("" or "0" = off, the default:
# nothing is launched, the result gains no key and every file keeps its bytes).
MESH_PREVIEW_VIEWS = _non_negative_int("O2345_MESH_PREVIEW_VIEWS", os.environ.get("O2345_MESH_PREVIEW_VIEWS", ""))


def mesh_preview_views(n=None):
    """None -> the configured default; anything else must be a non-negative integer (an explicit 0 is off whatever the default)."""
    if n is None:
        return MESH_PREVIEW_VIEWS
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"mesh_preview_views must be a non-negative integer, got {n!r}")
    return int(n)


# O2345_TEXTURED_PREVIEW_VIEWS=n makes pipeline.reconstruct_folder render the TEXTURED asset as a viewer shows it (the atlas sampled bilinearly, the normal
# map through the file's tangent frames, a headlight; csrc/mesh_raster.hip: k_rs_shade_tex) from the same cameras and write textured_000.png ... and
# textured_lit_000.png ... next to the PLY ("" or "0" = off, the default: nothing is launched, the result gains no key and every file keeps its bytes).  It
# needs a texture atlas (texture_texel) and an asset output format.
TEXTURED_PREVIEW_VIEWS = _non_negative_int("O2345_TEXTURED_PREVIEW_VIEWS", os.environ.get("O2345_TEXTURED_PREVIEW_VIEWS", ""))


def textured_preview_views(n=None):
    """None -> the configured default; anything else must be a non-negative integer (an explicit 0 is off whatever the default)."""
    if n is None:
        return TEXTURED_PREVIEW_VIEWS
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"textured_preview_views must be a non-negative integer, got {n!r}")
    return int(n)


def preview_views(n=None):
    """None -> the configured default; anything else must be a non-negative integer (an explicit 0 is off whatever the default)."""
    if n is None:
        return PREVIEW_VIEWS
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"preview_views must be a non-negative integer, got {n!r}")
    return int(n)
