"""What the timing tools of the fine training layers and of the trainable matcher share (imported by the time_* and
probe_* tools next to it; nothing runs here by itself): `say` prints a line and keeps it for the tool's --out file,
`write_log` writes that file, `timeit` is the device-event timer."""
import torch

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def write_log(path):
    """every line said so far -> `path` (no-op for None: the tool ran without --out)"""
    if path:
        with open(path, "w") as f:
            f.write("\n".join(LINES) + "\n")


def timeit(fn):
    """ms per call by device events, over a window of about 0.3 s (5 to 1000 calls)"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    torch.cuda.synchronize()
    n = int(min(1000, max(5, 300.0 / max(e0.elapsed_time(e1) / 3, 1e-3))))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
