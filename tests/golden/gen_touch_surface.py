#!/usr/bin/env python3
"""What the touch families (box, tri, obox, capsule, frustum) show to a caller, recorded so that a change to how their entries,
twins and bindings are written can be held to "nothing a caller sees moved" (tests/test_touch_surface.py replays both):

  entry_texts(lib, host)   every touch C entry of a device library (30) and of the host library (18) against each broken argument
                           rule - a null scene or description, kind 7, each buffer null in turn, each buffer off by one byte in
                           turn, n just past the per-launch limit (device entries) - and n == 0 with wild pointers: the return
                           code and the full error text. No call gets past the rules: the scene handle is a zeroed buffer that is
                           never read, and every call breaks a rule or has n == 0. The twins, which take buffers at any address, run
                           their one-item calls on an empty description, and one on a description they refuse by name.
  python_surface()         the names and inspect.signature strings of the module-level twins and the IpuScene attributes of the
                           families, and the values of their constants.

Run as a script it writes tests/golden/touch_entry_texts.json and tests/golden/touch_python_surface.json from the checkout it
lies in; the committed files were written by the commit BEFORE the families' entries became templates.

    python3 tests/golden/gen_touch_surface.py
"""
import ctypes as C
import inspect
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
import ipu_ray_lib_amd as irl  # noqa: E402

FAMILIES = ("box", "tri", "obox", "capsule", "frustum")
WITH_BOUNDS_TWIN = ("obox", "capsule", "frustum")
PAST_LIMIT = 0xFFBFFFFF + 1          # kMaxWorkItems + 1
WILD = 0xDEAD0001                    # odd, unmapped
ANY, COUNT = 0, 1


def _cases(names, good, kinds=(None,), limit=True):
    """(label, kind, pointers by name, n) of an entry whose buffers are `names`: each rule broken once, the others kept."""
    out = []
    for kind in kinds:
        tag = "" if kind is None else f"kind {kind}, "
        out.append((tag + "null scene", kind, dict(good, scene=None), 4))
        for b in names:
            out.append((tag + f"null {b}", kind, dict(good, **{b: None}), 4))
        for b in names:
            if b == "out" and kind == ANY:      # the bytes of ANY lie anywhere: no rule to break, and nothing may get past the rules
                continue
            out.append((tag + f"{b} off by one byte", kind, dict(good, **{b: good[b] + 1}), 4))
        if limit:
            out.append((tag + "n past the limit", kind, good, PAST_LIMIT))
        out.append((tag + "n == 0, wild pointers", kind, dict(good, **{b: WILD for b in names}), 0))
    if kinds != (None,):
        out.append(("kind 7", 7, good, 4))
        out.append(("kind 7, n == 0, null buffers", 7, dict(good, **{b: None for b in names}), 0))
    return out


def entry_texts(lib, host):
    """{"device": rows, "host": rows}, a row = [entry, case, return code, error text ("" when the call returns 0)]."""
    fake = C.create_string_buffer(4096)
    bufs = {name: irl.aligned_bytes(4096) for name in ("items", "out", "offsets", "hits")}
    good = {name: b.ctypes.data for name, b in bufs.items()}
    good["scene"] = C.cast(fake, C.c_void_p)
    rows = {"device": [], "host": []}

    def row(which, entry, case, rc, err):
        rows[which].append([entry, case, int(rc), err().decode() if rc else ""])

    for p in FAMILIES:
        for suffix, host_entry in (("_device", False), ("", True)):
            tail = (None,) if not host_entry else ()
            for label, kind, a, n in _cases(("items", "out"), good, kinds=(ANY, COUNT), limit=not host_entry):
                row("device", f"mi_{p}_query{suffix}", label, getattr(lib, f"mi_{p}_query{suffix}")(a["scene"], kind, a["items"], a["out"], n, *tail), lib.mi_last_error)
            for label, _, a, n in _cases(("items", "offsets"), good, limit=not host_entry):
                row("device", f"mi_{p}_offsets{suffix}", label, getattr(lib, f"mi_{p}_offsets{suffix}")(a["scene"], a["items"], a["offsets"], n, *tail), lib.mi_last_error)
            for label, _, a, n in _cases(("items", "offsets", "hits"), good, limit=not host_entry):
                row("device", f"mi_{p}_fill{suffix}", label, getattr(lib, f"mi_{p}_fill{suffix}")(a["scene"], a["items"], a["offsets"], a["hits"], 64, n, *tail),
                    lib.mi_last_error)
    assert bytes(fake.raw) == bytes(4096) and not any(b.any() for b in bufs.values()), "a call got past the argument rules"

    empty, refused = irl.SceneDesc(), irl.SceneDesc()
    refused.num_nodes = 1                        # and no nodes: walkTable refuses it in the entry's name
    good["scene"] = C.pointer(empty)
    visits = (C.c_uint64 * 2)()
    for p in FAMILIES:
        for label, kind, a, n in _cases(("items", "out"), good, kinds=(ANY, COUNT), limit=False) + [("refused description", COUNT, dict(good, scene=C.pointer(refused)), 1)]:
            row("host", f"mi_{p}_query_host", label, getattr(host, f"mi_{p}_query_host")(a["scene"], kind, a["items"], a["out"], min(n, 1), visits), host.mi_host_last_error)
        for label, _, a, n in _cases(("items", "offsets"), good, limit=False) + [("refused description", None, dict(good, scene=C.pointer(refused)), 1)]:
            row("host", f"mi_{p}_offsets_host", label, getattr(host, f"mi_{p}_offsets_host")(a["scene"], a["items"], a["offsets"], min(n, 1), visits), host.mi_host_last_error)
        for label, _, a, n in _cases(("items", "offsets", "hits"), good, limit=False) + [("refused description", None, dict(good, scene=C.pointer(refused)), 1)]:
            row("host", f"mi_{p}_fill_host", label, getattr(host, f"mi_{p}_fill_host")(a["scene"], a["items"], a["offsets"], a["hits"], 64, min(n, 1), visits),
                host.mi_host_last_error)
        if p in WITH_BOUNDS_TWIN:                # returns 0 or 1 and sets no text: an item of zeros is not walked
            entry = getattr(host, f"mi_{p}_meets_bounds_host")
            i, lo, hi = good["items"], good["out"], good["offsets"]
            for label, args in (("null item", (None, lo, hi)), ("null mn", (i, None, hi)), ("null mx", (i, lo, None)), ("item off by one byte", (i + 1, lo, hi)),
                                ("mn off by one byte", (i, lo + 1, hi)), ("mx off by one byte", (i, lo, hi + 1))):
                rows["host"].append([f"mi_{p}_meets_bounds_host", label, int(entry(*args)), ""])
    return rows


def _belongs(name):
    """Whether a public name of the module or of IpuScene is one of the five families'."""
    words = set(name.lower().split("_"))
    return bool(words & {"box", "obox", "oboxes", "capsule", "frustum", "tri", "touches", "overlaps", "contacts", "overlap", "contact", "cull", "voxelize", "collides"})


def python_surface():
    """{"module": {name: signature or repr of the value}, "IpuScene": {name: signature}} of the families' public names."""
    def show(obj):
        return str(inspect.signature(obj)) if callable(obj) else repr(obj)
    return {"module": {n: show(getattr(irl, n)) for n in sorted(vars(irl)) if not n.startswith("_") and _belongs(n)},
            "IpuScene": {n: show(getattr(irl.IpuScene, n)) for n in sorted(dir(irl.IpuScene)) if not n.startswith("_") and _belongs(n)}}


if __name__ == "__main__":
    texts = entry_texts(irl.device_lib(False), irl.host_lib())
    assert texts["device"] == entry_texts(irl.device_lib(True), irl.host_lib())["device"], "the two device builds disagree"
    (HERE / "touch_entry_texts.json").write_text(json.dumps(texts, indent=0) + "\n")
    (HERE / "touch_python_surface.json").write_text(json.dumps(python_surface(), indent=1, sort_keys=True) + "\n")
    print(len(texts["device"]), "device rows,", len(texts["host"]), "host rows,", {k: len(v) for k, v in python_surface().items()}, "names")
