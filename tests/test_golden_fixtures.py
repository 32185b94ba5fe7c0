"""The committed fixtures stay within the 1 MiB a committed file may take: the long-trajectory fixtures G9 / G10 are stored as
<name>.part<K>.npz (tests/tools/golden_io.py) and load as one record through the ``golden`` fixture."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_no_fixture_file_exceeds_one_mib():
    for f in os.listdir(GOLDEN):
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20, f


def test_long_fixtures_load_whole_from_their_parts(golden):
    for name, n_rir in (("g9_long", 8), ("g10_long_pose", 16)):
        g = golden(name)
        assert int(g["steps"]) == 1000 and g["curves"].shape == (1000, 7)
        assert g["stft"].shape == g["gt_stft"].shape == (n_rir, 60, 1, 513) and g["stft"].dtype == np.float32
        for p in g["probes"]:
            pre = "probe_" if str(p) == "params16" else f"probe_{p}_"
            assert g[pre + "stft"].shape == (n_rir, 60, 1, 513) and g[pre + "image"].shape == (32, 48, 3)
