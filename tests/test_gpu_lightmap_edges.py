"""The lightmap kernels on the cases of tests/_lightmap_edge_cases.py, through the engine-less forms
``engine.lightmap_surfels_device`` and ``engine.lightmap_resolve``: the device against the numpy model, on uint32 views.

  owners   equal to the model's in every word, in every family -- the model has no tile skip, no scan and no search;
  surfels  all eight words equal to the model's for ``mesh`` in {None, 0} and both values of ``flip``.  In the families c and g a
           word that is a NaN in the model must be a NaN on the device, of any sign and payload (section 17.1; the rule of
           sections 13 and 19.1, ``_probe_edge_cases.mismatches``); every other word is equal in every bit.  The families a, b, d
           and e hold no NaN -- asserted on the model first -- and are compared with no exception;
  pieces   the families a and d under forced cover pieces of 1 and 61 units: not a word changes;
  resolve  family f for ``dilate`` in {0, 1, 2, 3, 5, 64} under the same rule (the engine-less form writes a buffer of its own:
           the binding has no in-place form);
  engine   family d's longest list through ``Engine.lightmap_surfels`` equals the engine-less form.

tests/test_lightmap_edges_model.py holds the model to exact arithmetic on the same cases.
"""
import numpy as np
import pytest

from renderbaby_amd import abi, engine, lightmap
from tests import _lightmap_edge_cases as lec
from tests import _lightmap_scenes as lms
from tests._probe_edge_cases import mismatches, words
from tests.conftest import has_gpu
from tests.test_gpu_query import _engine

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
NO = abi.LIGHTMAP_NO_OWNER
NAN_FAMILIES = ("c far corners", "g surfels out of range")


def compare(got, want, where, nan_rule):
    """owners in every word; surfels in every word but the model's NaNs under ``nan_rule``.  Returns the NaN words compared and
    how many of them have the model's bits on the device as well."""
    (gs, go), (ws, wo) = got, want
    assert go.dtype == np.uint32 and go.shape == wo.shape and gs.shape == ws.shape, where
    bad = np.nonzero(go != wo)[0]
    assert len(bad) == 0, (where, "owners", len(bad), bad[:5], go[bad[:5]], wo[bad[:5]])
    bad, nans = mismatches(gs, ws, 8, nan_rule=nan_rule)
    assert len(bad) == 0, (where, "surfels", len(bad), bad[:5], gs[bad[:5]], ws[bad[:5]])
    g, w = words(gs, 8), words(ws, 8)
    return np.array([nans, int((g == w)[np.isnan(w.view(f32))].sum())])


@pytest.mark.parametrize("family", list(lec.FAMILIES))
def test_generator_equals_the_model(family):
    nan_rule = family in NAN_FAMILIES
    nans, owned = np.zeros(2, np.int64), 0
    for index, (name, tris, uvs, width, height) in enumerate(lec.cases(family)):
        if max(width, height) > abi.LIGHTMAP_MAX_SIDE:   # 1 x 70001 and 70001 x 1: the model's alone; the entry point refuses them
            with pytest.raises(engine.RenderError, match="InvalidOptions"):
                engine.lightmap_surfels_device(tris, uvs, width, height, device=0)
            continue
        for mesh in (None, 0):
            for flip in (False, True):
                want = lec.model(family, index, mesh, flip)
                if not nan_rule:
                    assert family in lec.NO_NAN_FAMILIES and not np.isnan(want[0].view(f32)).any(), (family, name)
                got = engine.lightmap_surfels_device(tris, uvs, width, height, mesh=mesh, flip=flip, device=0)
                nans += compare(got, want, (family, name, mesh, flip), nan_rule)
                owned += int((got[1] != NO).sum())
    print(f"{family}: {len(lec.cases(family))} cases, {owned} owned texels compared, {nans[0]} NaN words compared under the rule, {nans[1]} of them with the model's bits")
    assert owned > 0
    if family == "g surfels out of range":
        assert nans[0] > 0, "family g made no NaN"


@pytest.mark.parametrize("units", ["1", "61"])
@pytest.mark.parametrize("family", ["a slivers", "d long lists"])
def test_cover_pieces_change_no_word(family, units, monkeypatch):
    monkeypatch.setenv("RB_LIGHTMAP_PIECE_UNITS", units)
    for index, (name, tris, uvs, width, height) in enumerate(lec.cases(family)):
        got = engine.lightmap_surfels_device(tris, uvs, width, height, device=0)
        compare(got, lec.model(family, index), (family, name, "pieces of", units), False)


@pytest.mark.parametrize("dilate", [0, 1, 2, 3, 5, 64])
def test_resolve_equals_the_model(dilate):
    nans, failed = 0, []
    for name, sums, width, height in lec.cases("f resolve records"):
        got = engine.lightmap_resolve(sums, width, height, dilate, device=0)
        want = lightmap.resolve(sums, width, height, dilate)
        assert got.shape == want.shape == (height, width, 4)
        bad, n = mismatches(got, want, 4, nan_rule=True)
        if len(bad):
            failed.append((name, len(bad), bad[:5], got.reshape(-1, 4)[bad[:2]], want.reshape(-1, 4)[bad[:2]]))
        nans += n
    print(f"dilate {dilate}: {nans} NaN words compared under the rule")
    assert not failed, (dilate, len(failed), [f[0] for f in failed], failed[0])
    assert nans > 0


def test_the_engine_form_on_the_longest_list():
    name, tris, uvs, width, height = lec.cases("d long lists")[0]
    e = _engine(lms.uv_scene(tris, uvs, n_meshes=2))
    try:
        for mesh, flip in ((None, False), (0, True)):
            want = engine.lightmap_surfels_device(tris, uvs, width, height, mesh=mesh, flip=flip, device=0)
            compare(e.lightmap_surfels(width, height, mesh=mesh, flip=flip), want, (name, "engine", mesh, flip), False)
    finally:
        e.close()
