"""config.mesh_options: the one place where the mesh path's options are resolved (no GPU)."""
import importlib

import pytest

config = importlib.import_module("one-2-3-45_amd.config")

CONSTANTS = dict(MESH_MIN_COMPONENT_FACES=7, MESH_KEEP_LARGEST=True, MESH_DECIMATE_CELL=3.0, MESH_PROJECT_ITERATIONS=5, MESH_SMOOTH_ITERATIONS=6,
                 MESH_TEXTURE_TEXEL=8)


@pytest.fixture()
def configured(monkeypatch):
    for k, v in CONSTANTS.items():
        monkeypatch.setattr(config, k, v)
    monkeypatch.setattr(config, "MESH_PROJECT_MAX_MOVE", None)


def test_none_takes_the_constant_as_set_at_call_time(configured, monkeypatch):
    assert config.mesh_options() == config.MeshOptions(7, True, 3.0, 5, 3.0, 6, 8)
    monkeypatch.setattr(config, "MESH_SMOOTH_ITERATIONS", 1)
    monkeypatch.setattr(config, "MESH_KEEP_LARGEST", False)
    o = config.mesh_options()
    assert (o.smooth_iterations, o.keep_largest) == (1, False)
    with pytest.raises(AttributeError):
        o.smooth_iterations = 2                    # a record, not a bag


def test_an_explicit_value_wins_and_zero_is_off(configured):
    o = config.mesh_options(min_component_faces=2, keep_largest=False, decimate_cell=1.5, project_iterations=1, smooth_iterations=2, texture_texel=4)
    assert o == config.MeshOptions(2, False, 1.5, 1, 1.5, 2, 4)
    assert type(o.decimate_cell) is float and type(o.min_component_faces) is int
    off = config.mesh_options(min_component_faces=0, keep_largest=False, decimate_cell=0, project_iterations=0, smooth_iterations=0, texture_texel=0)
    assert off == config.MeshOptions(0, False, 0.0, 0, 1.0, 0, 0) and not any(off[:4]) and not any(off[5:])
    # one explicit option leaves the others at their constants
    assert config.mesh_options(smooth_iterations=0) == config.MeshOptions(7, True, 3.0, 5, 3.0, 0, 8)


def test_the_move_limit_follows_this_calls_cell(configured, monkeypatch):
    assert config.mesh_options().project_max_move == 3.0                               # max(1, configured cell)
    assert config.mesh_options(decimate_cell=0.25).project_max_move == 1.0             # never below one spacing
    assert config.mesh_options(decimate_cell=2).project_max_move == 2.0
    assert config.mesh_options(decimate_cell=0).project_max_move == 1.0
    monkeypatch.setattr(config, "MESH_PROJECT_MAX_MOVE", 0.75)                         # configured: whatever the cell
    assert config.mesh_options(decimate_cell=2).project_max_move == 0.75 and config.mesh_options().project_max_move == 0.75


@pytest.mark.parametrize("option,resolver,bad", [
    ("min_component_faces", "mesh_min_component_faces", (-1, 1.5, True)),
    ("decimate_cell", "mesh_decimate_cell", (-1.0, float("nan"), float("inf"))),
    ("project_iterations", "mesh_project_iterations", (-1, 65, 2.5, True)),
    ("smooth_iterations", "mesh_smooth_iterations", (-1, 0.5, False)),
    ("texture_texel", "mesh_texture_texel", (3, 65, -4, 4.5, True)),
])
def test_an_invalid_value_raises_what_its_validator_raises(option, resolver, bad):
    for value in bad:
        with pytest.raises(ValueError) as want:
            getattr(config, resolver)(value)
        with pytest.raises(ValueError) as got:
            config.mesh_options(**{option: value})
        assert str(got.value) == str(want.value)
