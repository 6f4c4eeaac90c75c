"""Every status the host half of the coarse training entry points decides (csrc/dsm_grad.hip: dsm_status), the sibling
of tools/window_status_sweep.py: fm_dual_softmax_conf_at, fm_dual_softmax_backward, fm_dual_softmax_backward_dense,
fm_coarse_loss_forward and fm_coarse_loss_backward.  For one valid argument row per form (K > 0 and K = 0, with and
without id lists; the loss calls with both kinds) the tool prints what the library answers to the row itself, to every
single defect and to every pair of defects from different classes (which pins the precedence), then the two workspace
queries on a fixed list of shapes.  Two builds whose entry points check and size alike print the same text:
    python tools/dsm_status_sweep.py [--lib PATH] > sweep.txt

Pointers are C.c_void_p(256), never dereferenced: a row is answered by the argument checks.  A row that passes them goes
on to its first launch, so the tool hides every GPU from its own process first: the launch then fails with the
runtime's no-device error and the row is shown as L.  One line per (form, first defect): a letter per second defect,
grouped by class in the order of the form's header line.  O = FM_OK, N = FM_E_NULL, S = FM_E_SHAPE,
U = FM_E_UNSUPPORTED, W = FM_E_WORKSPACE, L = passed the checks, . = the same argument twice (no row)."""
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

HEAD = "feat0 feat1 N L S C temperature ofs_r sum_r pitch_r ofs_c sum_c pitch_c "
LOSS = "kind alpha gamma pos_weight neg_weight b_ids i_ids j_ids K workspace workspace_bytes "
ARGS = {
    "fm_dual_softmax_conf_at": HEAD + "b_ids i_ids j_ids K conf stream",
    "fm_dual_softmax_backward": HEAD + "b_ids i_ids j_ids gc K workspace workspace_bytes d_feat0 d_feat1 stream",
    "fm_dual_softmax_backward_dense": HEAD + "G workspace workspace_bytes d_feat0 d_feat1 stream",
    "fm_coarse_loss_forward": HEAD + LOSS + "loss_out stream",
    "fm_coarse_loss_backward": HEAD + LOSS + "d_loss d_feat0 d_feat1 stream",
}
PLAIN = dict(N=1, L=100, S=90, C=64, temperature=0.1, pitch_r=128, pitch_c=128, K=8, kind=_lib.FM_LOSS_FOCAL, alpha=0.25,
             gamma=2.0, pos_weight=1.0, neg_weight=1.0, stream=None)
NO_LISTS = dict(K=0, b_ids=None, i_ids=None, j_ids=None)
K_FORMS = [{}, dict(K=0), NO_LISTS]
FORMS = {        # entry point -> the changes to its default row that make each form
    "fm_dual_softmax_conf_at": K_FORMS,
    "fm_dual_softmax_backward": K_FORMS + [dict(NO_LISTS, gc=None)],
    "fm_dual_softmax_backward_dense": [{}],
    "fm_coarse_loss_forward": [dict(a, kind=k) for k in (_lib.FM_LOSS_FOCAL, _lib.FM_LOSS_CROSS_ENTROPY) for a in K_FORMS],
    "fm_coarse_loss_backward": [dict(a, kind=k) for k in (_lib.FM_LOSS_FOCAL, _lib.FM_LOSS_CROSS_ENTROPY) for a in K_FORMS],
}
LETTER = {0: "O", -1: "N", -2: "S", -3: "U", -4: "W"}
SHAPES = [(1, 100, 90, 64), (1, 4800, 4800, 256), (2, 255, 143, 128), (64, 4800, 4800, 256), (1, 1, 1, 4), (2, 300, 192, 100),
          (3, 33, 31, 36), (1, 1200, 1200, 8)]


def need(name, row):
    shape = (row["N"], row["L"], row["S"], row["C"])
    if "loss" in name:
        return int(LIB.fm_coarse_loss_workspace_bytes(*shape, row["K"]))
    return int(LIB.fm_dual_softmax_backward_workspace_bytes(*shape))


def defects(name, row):
    """[(class, label, {argument: value})] of a form's row, in a fixed order"""
    out = [("null", k, {k: None}) for k, v in row.items() if isinstance(v, C.c_void_p)]
    out += [("size", f"{k}={bad}", {k: bad}) for k in ("N", "L", "S") for bad in (0, -3)]
    if "K" in row:
        out += [("size", "K=-1", dict(K=-1)), ("size", "K=N*L*S+1", dict(K=row["N"] * row["L"] * row["S"] + 1))]
    out += [("size", f"pitch_r={row['L'] - 1}", dict(pitch_r=row["L"] - 1)), ("size", f"pitch_c={row['S'] - 1}", dict(pitch_c=row["S"] - 1))]
    out += [("C", f"C={v}", dict(C=v)) for v in (0, 6, 260)]
    out += [("temperature", f"temperature={v}", dict(temperature=v)) for v in (0.0, -1.0, float("nan"))]
    if "kind" in row:
        out += [("kind/gamma", f"kind={v}", dict(kind=v)) for v in (2, -1)]
        out += [("kind/gamma", f"gamma={v}", dict(gamma=v)) for v in (0.0, -2.0)]
    if "workspace" in row:
        out += [("workspace", "workspace_bytes=need-1", dict(workspace_bytes=row["workspace_bytes"] - 1)),
                ("workspace", "workspace_bytes=16", dict(workspace_bytes=16)),
                ("workspace", "workspace=264", dict(workspace=C.c_void_p(264)))]
    return out


def status(name, row, *changes):
    args = dict(row)
    for ch in changes:
        args.update(ch)
    return LETTER.get(getattr(LIB, name)(*args.values()), "L")


rows = 0
for name, arg_names in ARGS.items():
    kinds = _lib.SIGNATURES[name][1]
    names = arg_names.split()
    assert len(names) == len(kinds), name
    base = {k: PLAIN[k] if k in PLAIN else C.c_void_p(256) if kind is C.c_void_p else 0 for k, kind in zip(names, kinds)}
    for form in FORMS[name]:
        assert set(form) <= set(base), (name, form)
        row = dict(base, **form)
        if "workspace" in row:
            row["workspace_bytes"] = need(name, row)            # exactly what the query asks for
        ds = defects(name, row)
        classes = [c for c, _ in itertools.groupby(ds, key=lambda d: d[0])]
        shown = {k: ("NULL" if v is None else "ptr" if isinstance(v, C.c_void_p) else v) for k, v in row.items()}
        print(f"# {name} " + " ".join(f"{k}={v}" for k, v in shown.items()))
        for c in classes:
            print(f"#   {c}: " + " ".join(d[1] for d in ds if d[0] == c))
        print(f"valid {status(name, row)}")
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
print("# workspace bytes: N L S C | fm_dual_softmax_backward_workspace_bytes | fm_coarse_loss_workspace_bytes at K = 0, 1, 100, 5000")
for shape in SHAPES:
    sizes = [int(LIB.fm_coarse_loss_workspace_bytes(*shape, k)) for k in (0, 1, 100, 5000)]
    print(*shape, "|", int(LIB.fm_dual_softmax_backward_workspace_bytes(*shape)), "|", *sizes)
