"""GPU box: in-kernel wall-clock stamps (100 MHz) of the preprocessing kernels (csrc/kpf_prep.hip), one row per sample of a mixed B = 32 batch: where
kpf_prep_crop_u16 and kpf_prep_pcl_sample spend their time, phase by phase, against the number of candidates N the sort runs over.
usage: python tools/prep_stamps.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import prep_cases as PC  # noqa: E402
from keypointfusion_amd import lib as L  # noqa: E402
from keypointfusion_amd.preprocess_gpu import DevicePreprocessor  # noqa: E402

dev = torch.device("cuda:0")
names = list(PC.CASES)
B = 32
fr = [PC.synth_frame(names[i % len(names)]) for i in range(B)]
ins = (torch.from_numpy(np.stack([f[0] for f in fr])).to(dev), torch.from_numpy(np.stack([f[1] for f in fr])).to(dev),
       torch.tensor([f[2] for f in fr], dtype=torch.float64, device=dev), torch.tensor([f[3] for f in fr], dtype=torch.float64, device=dev),
       torch.arange(B, dtype=torch.int64, device=dev))
pre = DevicePreprocessor()
lib = L.load()
for _ in range(3):
    prep = pre.prepare(*ins)
torch.cuda.synchronize()
st = torch.zeros(B, 8, dtype=torch.int64, device=dev)
L.check(lib.kpf_prep_set_stamps(st.data_ptr()))
prep = pre.prepare(*ins)
torch.cuda.synchronize()
L.check(lib.kpf_prep_set_stamps(None))
s = st.cpu().numpy().astype(np.float64) / 100.0  # microseconds
N = prep["pcl_count"].cpu().numpy()
print("%-16s %6s | crop: %9s %8s %9s | sample: %8s %8s %8s  (microseconds)" % ("case", "N", "com+geom", "gather", "normalise", "compact", "sort", "points"))
for b in range(len(names)):
    print("%-16s %6d | %15.1f %8.1f %9.1f | %16.1f %8.1f %8.1f" % (names[b], N[b], s[b, 1] - s[b, 0], s[b, 2] - s[b, 1], s[b, 3] - s[b, 2],
                                                                    s[b, 5] - s[b, 4], s[b, 6] - s[b, 5], s[b, 7] - s[b, 6]))
print("launch spans: crop %.1f us, sample %.1f us" % (s[:, 3].max() - s[:, 0].min(), s[:, 7].max() - s[:, 4].min()))
