"""Writes tests/golden/ssim_bits.json: the fp64 bit patterns `ops.image_metrics` and `ops.image_ssim` give on the cases of tests/ssim_bits_cases.py.
tests/test_ssim_bits_gpu.py asserts that the library reproduces every pattern, so run this at the commit whose bits are the promise (the parent of a change
to the SSIM kernels), never at the code under test.

    python tools/gen_ssim_bits.py [--out tests/golden/ssim_bits.json]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import ssim_bits_cases as SB
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", SB.FIXTURE))
ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
if a.commit is None:
    try:
        a.commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        a.commit = "unknown"
res = {"generated_by": "tools/gen_ssim_bits.py", "commit": a.commit, "device": torch.cuda.get_device_name(0), "B": SB.B}
res.update(SB.run(ops, torch, dev))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(json.dumps(res, indent=0) + "\n")
print(f"{a.out}: {len(res['image_metrics'])} image_metrics and {len(res['image_ssim'])} image_ssim cases", flush=True)
