"""What the stage perf tools (dmrs_perf.py, eq_perf.py, demod_perf.py, rm_perf.py, tp_perf.py) share: the common arguments, the device
check, the event timing of LAUNCHES launches, the spread line, and the print-and-write tail.  Each tool keeps its own
shapes, its (a)/(b)/(c) definitions and its line formats."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]


def parser(doc, tool, rehearse_help="host logic only; no GPU, nothing measured, nothing written"):
    """ArgumentParser with --launches / --repeats / --out (profiles/<tool>.txt) / --rehearse; the tool adds its own."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20, help="launches per repeat of the device timings (>= 20)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / f"{tool}.txt"))
    ap.add_argument("--rehearse", action="store_true", help=rehearse_help)
    return ap


def stats(xs, width=8):
    return f"mean {statistics.mean(xs):{width}.4f} ms  min {min(xs):{width}.4f}  max {max(xs):{width}.4f}  (n={len(xs)})"


def gpu(tool):
    """cuda:0, or exit: the measurements need a GPU."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"tools/{tool}.py measures on a GPU; none is visible (use --rehearse for the host logic)")
    return torch.device("cuda:0")


def timed(fn, n):
    """Mean milliseconds of n back-to-back calls of fn on the current stream, between two device events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def finish(lines, out):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(text)
