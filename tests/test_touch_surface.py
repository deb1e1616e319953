"""The touch families' entries, twins and bindings are written once per kind and stamped per family; what a caller sees of them is
held to what the hand-written ones showed. Both tests replay tests/golden/gen_touch_surface.py against this build and compare,
exactly, with the fixtures that generator wrote from the commit before the entries became templates. No GPU: no call gets past
the argument rules."""
import inspect
import json
import sys

import pytest

import ipu_ray_lib_amd as irl

GOLDEN = irl.REPO_ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import gen_touch_surface as gen  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return json.loads((GOLDEN / "touch_entry_texts.json").read_text())


@pytest.mark.parametrize("variants", [False, True])
def test_entry_texts_are_the_recorded_ones(recorded, variants):
    """Return code and full error text of all 30 device-library entries (both builds) and all 18 host-library entries, rule by rule."""
    got = gen.entry_texts(irl.device_lib(variants), irl.host_lib())
    for which in ("device", "host"):
        assert len({r[0] for r in recorded[which]}) == {"device": 30, "host": 18}[which]
        assert [tuple(r[:2]) for r in got[which]] == [tuple(r[:2]) for r in recorded[which]], "the enumeration itself moved"
        wrong = [(g, w) for g, w in zip(got[which], recorded[which]) if g != w]
        assert not wrong, f"{len(wrong)} of {len(got[which])} {which} rows differ, first (got, recorded): {wrong[0]}"


def _c_entries(name):
    """The C entries a public Python name of a family stands on: its docstring must name one of them."""
    p = next((q for q in ("obox", "capsule", "frustum", "tri", "box") if name.startswith(q + "_") or f"_{q}_" in name), None)
    if p is None:
        p = "tri" if "contacts" in name else "box"
    if name.endswith("_host"):
        return [f"mi_{name}"]
    for kind in ("query", "offsets", "fill"):
        if name == f"{p}_{kind}" or name == f"{p}_{kind}_device":
            return [f"mi_{name}"]
    if name.startswith(("list_", "first_")) or name.endswith("_list"):
        return [f"mi_{p}_fill", f"mi_{p}_offsets"]
    return [f"mi_{p}_query"]                      # touches, counts, the torch any / count


BUILT_ON_THEM = ("voxelize", "mesh_contacts", "collides", "cull")      # written in terms of the methods above: signatures only


def test_python_surface_is_the_recorded_one():
    want = json.loads((GOLDEN / "touch_python_surface.json").read_text())
    got = gen.python_surface()
    for scope in ("module", "IpuScene"):
        assert sorted(got[scope]) == sorted(want[scope]), (scope, set(got[scope]) ^ set(want[scope]))
        moved = {n: (got[scope][n], want[scope][n]) for n in want[scope] if got[scope][n] != want[scope][n]}
        assert not moved, f"{scope}: (now, recorded) {moved}"
    assert len(want["module"]) == 36 and len(want["IpuScene"]) == 64
    for scope, holder in (("module", irl), ("IpuScene", irl.IpuScene)):
        for name in want[scope]:
            obj = getattr(holder, name)
            if not callable(obj) or name in BUILT_ON_THEM:
                continue
            doc = inspect.getdoc(obj) or ""
            assert obj.__name__ == name and any(entry in doc for entry in _c_entries(name)), (scope, name, _c_entries(name), doc[:80])
