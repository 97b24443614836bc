"""CPU: tests/golden_store.py -- golden vectors stored in parts of at most 1 MiB come back bit for bit, in the order they were saved."""
import glob
import os

import numpy as np

from tests import golden_store

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_save_load_round_trip_in_small_parts(tmp_path):
    rng = np.random.RandomState(3)
    arrays = {"big": rng.rand(300, 1000).astype(np.float32), "u8": rng.randint(0, 255, (5, 400, 400, 3)).astype(np.uint8),
              "small": np.arange(7, dtype=np.int64), "scalar": np.int64(388)}
    stem = str(tmp_path / "vec")
    golden_store.save(stem, **arrays)
    files = glob.glob(stem + ".part*.npz")
    assert len(files) > 1 and all(os.path.getsize(f) < 1 << 20 for f in files)
    back = golden_store.load(stem)
    assert list(back) == list(arrays)
    for k, v in arrays.items():
        v = np.asarray(v)
        assert back[k].dtype == v.dtype and back[k].shape == v.shape and np.array_equal(back[k], v), k


def test_committed_goldens_stay_below_1_mib_and_load():
    assert all(os.path.getsize(f) < 1 << 20 for f in glob.glob(os.path.join(GOLDEN, "*")))
    z = golden_store.load(os.path.join(GOLDEN, "real388_heldout"))
    assert z["x"].shape[0] == z["y"].shape[0] == 4 and int(z["P"]) == 388
    pz = golden_store.load(os.path.join(GOLDEN, "real388_trained_params"))
    assert pz["conv_0__conv1__kernel"].shape[:2] == (3, 3) and all(v.dtype == np.float32 for v in pz.values())
    assert "color_space_adjust__kernel" in golden_store.load(os.path.join(GOLDEN, "real_crops_trained_params"))
