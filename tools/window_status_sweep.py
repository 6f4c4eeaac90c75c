"""Every status the host half of the window-call entry points decides: the forward crop / merge / fine-from-maps entry
points of csrc/fine.hip plus fm_gather_windows_backward.  For one valid argument row per form (one image / two images,
plain / merge, each layout and element type) the tool prints what the library answers to the row with m_max = 0, to
every single defect and to every pair of defects from different classes (which pins the precedence).  Two builds whose
entry points check alike print the same text:  python tools/window_status_sweep.py [--lib PATH] > sweep.txt

Pointers are C.c_void_p(256), never dereferenced: a row is answered by the argument checks.  A few "defects" are none
for some entry point (Cf = 32 for the generic crop, say); such a row passes the checks and goes on to its launch, so
the tool hides every GPU from its own process first: the launch then fails with the runtime's no-device error and the
row is shown as L.  One line per (form, first defect): a letter per second defect, grouped by class in the order of
the form's header line.  O = FM_OK, N = FM_E_NULL, S = FM_E_SHAPE, U = FM_E_UNSUPPORTED, W = FM_E_WORKSPACE,
L = passed the checks, . = the same argument twice (no row)."""
import argparse
import ctypes as C
import itertools
import os
import sys

os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = ""       # no row may reach a GPU
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from featurematching_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of the same ABI (default: the tree's own library)")
LIB = _lib.load(ap.parse_args().lib)

ONE_MAP = "feat_f {dt} N Cf Hf Wf {lay} W stride pad {hc} w_c {cells} {merge} b_ids ids d_count m_max out stream"
TWO_MAPS = "feat_f0 feat_f1 {head} N Cf Hf0 Wf0 Hf1 Wf1 W stride pad {grid} {mid} b_ids i_ids j_ids d_count m_max {tail} out0 out1 stream"
CELLS2 = "cell0 pitch0 ties0 cell1 pitch1 ties1"
FINE_TAIL = "mix0 mix1 mkpts0_c mkpts1_c scale_f scratch"
ARGS = {
    "fm_gather_windows": ONE_MAP.format(dt="", lay="layout", hc="", cells="", merge=""),
    "fm_gather_windows_dtype": ONE_MAP.format(dt="map_dtype", lay="layout", hc="", cells="", merge=""),
    "fm_gather_windows_cells": ONE_MAP.format(dt="", lay="", hc="h_c", cells="cell_to_match cell_pitch ties", merge=""),
    "fm_gather_merge_windows": ONE_MAP.format(dt="", lay="", hc="h_c", cells="cell_to_match cell_pitch ties",
                                              merge="packed_w ctx_bias"),
    "fm_gather_windows_pair": TWO_MAPS.format(head="", grid="h0c w0c h1c w1c", mid=CELLS2 + " packed_w ctx0 ctx1", tail=""),
    "fm_gather_merge_windows_nhwc": TWO_MAPS.format(head="map_dtype", grid="h0c w0c h1c w1c", mid="packed_w ctx0 ctx1", tail=""),
    "fm_fine_match_maps": TWO_MAPS.format(head="layout", grid="w0c w1c", mid="", tail=FINE_TAIL),
    "fm_fine_match_maps_dtype": TWO_MAPS.format(head="map_dtype layout", grid="w0c w1c", mid="", tail=FINE_TAIL),
    "fm_gather_windows_backward": "d_win b_ids ids d_count m_max N Cf Hf Wf layout W stride pad h_c w_c workspace "
                                  "workspace_bytes d_feat stream",
}
PLAIN = dict(N=1, Cf=64, W=7, stride=4, pad=2, m_max=3, layout=0, map_dtype=0, scale_f=2.0, workspace_bytes=1 << 40,
             d_count=None, stream=None)
LIST_ORDER = dict(cell_to_match=None, cell_pitch=0, ties=None)
NO_MERGE = dict(packed_w=None, ctx0=None, ctx1=None)
ONE_IMAGE = dict(feat_f1=None, ctx1=None, j_ids=None, out1=None, Hf1=0, Wf1=0, h1c=0, w1c=0)
LAYOUTS, DTYPES = [dict(layout=v) for v in (0, 1)], [dict(map_dtype=v) for v in (0, 1, 2)]
FORMS = {        # entry point -> the changes to its default row that make each form
    "fm_gather_windows": LAYOUTS,
    "fm_gather_windows_dtype": [dict(a, **b) for a in LAYOUTS for b in DTYPES],
    "fm_gather_windows_cells": [{}],
    "fm_gather_merge_windows": [{}, LIST_ORDER],
    "fm_gather_windows_pair": [NO_MERGE, {}],
    "fm_gather_merge_windows_nhwc": [dict(a, **b) for a in (ONE_IMAGE, {}) for b in DTYPES],
    "fm_fine_match_maps": LAYOUTS + [dict(layout=2)],
    "fm_fine_match_maps_dtype": [dict(a, **b) for a in LAYOUTS for b in DTYPES] + [dict(layout=2, map_dtype=0)],
    "fm_gather_windows_backward": LAYOUTS,
}
LETTER = {0: "O", -1: "N", -2: "S", -3: "U", -4: "W"}
BIG = (4096, 2048)          # Hf x Wf x 64 channels x 4 bytes = 2^31 bytes per sample


def default(name, kind):
    if name in PLAIN:
        return PLAIN[name]
    if kind is C.c_void_p:
        return C.c_void_p(256)
    return 8 if name[0] in "HW" else 4 if "pitch" in name else 2          # map 8 x 8, coarse grid 2 x 2, pitch = its cells


def defects(row):
    """[(class, label, {argument: value})] of a form's row, in a fixed order"""
    out = []
    for k, v in row.items():
        if isinstance(v, C.c_void_p):
            out.append(("null", k, {k: None}))
    for k, v in row.items():
        if k == "m_max":
            out.append(("size", "m_max=-3", {k: -3}))
        elif isinstance(v, int) and v > 0 and (k in ("N", "stride") or k[0] in "HWhw" and k != "W"):
            out += [("size", f"{k}={bad}", {k: bad}) for bad in (0, -3)]
    out += [("Cf", f"Cf={v}", dict(Cf=v)) for v in (0, 32, 128, 516)]
    out += [("W", f"W={v}", dict(W=v)) for v in (0, 3, 9, 15, 16)]
    out += [("layout", f"layout={v}", dict(layout=v)) for v in (-1, 2, 3) if "layout" in row and row["layout"] != v]
    out += [("dtype", f"map_dtype={v}", dict(map_dtype=v)) for v in (-1, 3) if "map_dtype" in row]
    out += [("pitch", f"{k}=3", {k: 3}) for k, v in row.items() if "pitch" in k and v]
    out += [("big", f"H{s}xW{s}=2^31B", {"H" + s: BIG[0], "W" + s: BIG[1]}) for s in ("f", "f0", "f1") if row.get("H" + s)]
    return out


def status(name, row, *changes):
    args = dict(row)
    for ch in changes:
        args.update(ch)
    st = getattr(LIB, name)(*args.values())
    return LETTER.get(st, "L")


rows = 0
for name, arg_names in ARGS.items():
    kinds = _lib.SIGNATURES[name][1]
    names = arg_names.split()
    assert len(names) == len(kinds), name
    base = {k: default(k, kind) for k, kind in zip(names, kinds)}
    for form in FORMS[name]:
        assert set(form) <= set(base), (name, form)
        row = dict(base, **form)
        ds = defects(row)
        classes = [c for c, _ in itertools.groupby(ds, key=lambda d: d[0])]
        shown = {k: ("NULL" if v is None else "ptr" if isinstance(v, C.c_void_p) else v) for k, v in row.items()}
        print(f"# {name} " + " ".join(f"{k}={v}" for k, v in shown.items()))
        for c in classes:
            print(f"#   {c}: " + " ".join(d[1] for d in ds if d[0] == c))
        print(f"m_max=0 {status(name, row, dict(m_max=0))}")
        rows += 1
        for ca, la, a in ds:
            cells = []
            for c in classes:
                if c == ca:
                    continue
                word = ""
                for cb, lb, b in ds:
                    if cb == c:
                        same = set(a) & set(b)
                        word += "." if same else status(name, row, a, b)
                        rows += 0 if same else 1
                cells.append(word)
            print(f"{la} {status(name, row, a)} | " + " ".join(cells))
            rows += 1
print(f"# rows {rows} (every pair is counted from both of its defects)")
