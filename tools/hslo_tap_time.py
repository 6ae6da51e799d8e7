"""The bottom-to-top scanline kernel's time on the C3 configuration (1080p, D = 64, stages 0x103), from stm_prof_read: one JSON line.
Run from the root of the tree to be measured (this tree, or a checkout of another commit with its library built), several times
each and alternately, to compare two commits -- profiles/hslo_tap_time.json holds such a comparison for the commit that put the
test tap's pointer test into the kernel.  usage: python tools/hslo_tap_time.py [frames]"""
import json
import os
import sys
import zlib

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
import stm_amd  # noqa: E402
from stm_amd import device_api as dev, synth  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 40
H, W, D, zd = 1080, 1920, 64, 32
sbs, _ = synth.sbs_frame(H, W, D, zd)
p = dev.FrameParams(num_disp=D, zero_disp=zd)
d_sbs = torch.from_numpy(sbs).cuda()
dl = torch.zeros(H, W, dtype=torch.float32, device="cuda")
dr = torch.zeros_like(dl)
out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
for _ in range(5):
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=0x103)
torch.cuda.synchronize()
dev.prof_reset()
dev.prof_enable(True)
for _ in range(frames):
    dev.d_adcensus_stm(d_sbs, dl, dr, out, p, stages=0x103)
torch.cuda.synchronize()
dev.prof_enable(False)
res = {"frames": frames}
for name in ("hslo_lr", "hslo_tb", "hslo_bt"):
    n, ms = dev.prof_read(name)
    res[name + "_us"] = round(1e3 * ms / max(n, 1), 2)
    res[name + "_launches"] = n
res["crc"] = "%08x" % (zlib.crc32(dl.cpu().numpy().tobytes()) ^ zlib.crc32(dr.cpu().numpy().tobytes()) ^ zlib.crc32(out.cpu().numpy().tobytes()))
print(json.dumps(res), flush=True)
