"""Golden sample of the BoxDiff energy goldens' INPUT maps: tests/golden/boxdiff_energy.npz stores no maps (they are
regenerated from their seeds by tests/boxdiff_maps.py) and only a float64 checksum of each case's first map, which is
exact on the CPU vector ISA that recorded it and off in the last bits elsewhere (ATen's AVX2 and AVX-512 soft-max / exp
kernels round differently).  This writes, per case and key, the values of the regenerated maps at 256 fixed, seeded
positions, which tests/test_boxdiff_cpu.py compares within fp32 round-off on any host.

    python oracle/make_golden_boxdiff_maps.py    # writes tests/golden/boxdiff_maps_sample.npz

It refuses to write unless every regenerated first map reproduces the recorded checksum bit for bit, i.e. unless the
sample is of the very maps the energy goldens were computed from.  Needs no reference checkout."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "..", "tests", "golden")
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from boxdiff_maps import KEYS, make_maps  # noqa: E402

N_SAMPLE = 256

g = np.load(os.path.join(GOLD, "boxdiff_energy.npz"))
names = sorted(k[:-len("_spec")] for k in g.files if k.endswith("_spec"))
outs = {}
for name in names:
    spec = json.loads(str(g[f"{name}_spec"]))
    maps = make_maps(spec["side"], spec["heads"], spec["seed"])
    checksum = float(maps[tuple(KEYS[0])].double().sum())
    if checksum != float(g[f"{name}_map0_checksum"]):
        raise SystemExit(f"{name}: regenerated maps differ from the golden's inputs (checksum {checksum!r}); run this on "
                         "a host whose CPU kernels reproduce them (the recorded checksums were taken with AVX-512)")
    size = maps[tuple(KEYS[0])].numel()
    idx = np.sort(np.random.default_rng(0).choice(size, N_SAMPLE, replace=False))
    outs[f"{name}_idx"] = idx
    outs[f"{name}_values"] = np.stack([maps[tuple(k)].reshape(-1).numpy()[idx] for k in KEYS])     # [keys, N_SAMPLE]
np.savez_compressed(os.path.join(GOLD, "boxdiff_maps_sample.npz"), **outs)
print("wrote boxdiff_maps_sample.npz:", ", ".join(names))
