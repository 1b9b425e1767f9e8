"""End-to-end cost of ``main.py --occlusion`` on the synthetic 200 x 200 JPEG set of tools/e2e_5000.py (same generator, same seed):
    python tools/e2e_occlusion.py [n_images] [batch]
Writes the set under $TMPDIR, runs vip-cup-2022_amd/main.py --synthetic plain (twice: the first run pays model build + page-in) and then
with --occlusion DIR at the defaults (8 x 8 cells, 2 x 2 windows: 49 variants per image), and prints the CLI's own "TIME TO INFER" lines,
the ratio of the two and the predicted 1 + 49."""
import os, re, shutil, subprocess, sys, tempfile
import numpy as np
from PIL import Image

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
batch = sys.argv[2] if len(sys.argv) > 2 else "256"
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
d = tempfile.mkdtemp(prefix="vipocc_")
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:200, 0:200].astype(np.float32)
names = []
for i in range(n):
    f = rng.uniform(0.01, 0.08, size=(3, 2))
    ph = rng.uniform(0, 6.28, size=3)
    img = np.stack([127 + 90 * np.sin(f[c, 0] * xx + f[c, 1] * yy + ph[c]) for c in range(3)], -1)
    img += rng.normal(0, 12, img.shape)
    name = f"img_{i:05d}.jpg"
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(d, name), quality=int(rng.integers(75, 96)),
                                                                 subsampling=int(rng.integers(0, 3)))
    names.append(name)
with open(os.path.join(d, "input.csv"), "w") as fh:
    fh.write("filename\n" + "\n".join(names) + "\n")
print(f"wrote {n} JPEGs to {d}", flush=True)
base = [sys.executable, os.path.join(root, "vip-cup-2022_amd", "main.py"), os.path.join(d, "input.csv")]
rates = {}
for label, extra in (("plain (cold)", []), ("plain", []), ("occlusion", ["--occlusion", os.path.join(d, "occ")])):
    out_csv = os.path.join(d, "out_occ.csv" if extra else "out.csv")
    r = subprocess.run(base + [out_csv, "--synthetic", "--batch-size", batch] + extra, capture_output=True, text=True)
    tail = [l for l in r.stdout.splitlines() if "TIME TO INFER" in l or "SAVED" in l]
    print(f"{label}: rc={r.returncode}", *tail, sep="\n  ", flush=True)
    if r.returncode != 0:
        print(r.stderr[-2000:])
        break
    m = re.search(r"\(([0-9.]+) images/s", r.stdout)
    rates[label] = float(m.group(1))
if "occlusion" in rates:
    same = open(os.path.join(d, "out.csv"), "rb").read() == open(os.path.join(d, "out_occ.csv"), "rb").read()
    t_plain, t_occ = n / rates["plain"], n / rates["occlusion"]
    files = len([f for f in os.listdir(os.path.join(d, "occ")) if f.endswith(".npy")])
    print(f"{n} images, batch {batch}: plain {t_plain:.2f} s ({rates['plain']:.1f} images/s), --occlusion {t_occ:.2f} s "
          f"({rates['occlusion']:.1f} images/s), ratio {t_occ / t_plain:.1f}x against the predicted 1 + 49 = 50x; "
          f"{files} maps written; output CSV identical: {same}")
shutil.rmtree(d, ignore_errors=True)
