"""Host logic of bench.py that needs no GPU: launch-set plans and the strong-scaling split of BASELINE.json configs[2]."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("steps", [1, 5, 8, 20, 32, 33, 64, 100, 384])
@pytest.mark.parametrize("streams", [1, 2, 3])
def test_plan_covers_every_step_once(bench, steps, streams):
    plan = bench.plan_batches(steps, streams, bench.MAX_BATCH)
    assert sum(plan) == steps and all(1 <= b <= bench.MAX_BATCH for b in plan)
    if steps <= 32:
        assert plan == [steps]  # a short run is ONE launch set


def test_dump_outputs_writes_the_packed_skeleton(bench, tmp_path):
    """--dump-outputs: the step's skeleton in sharding.pack_skeleton's layout, float64 branch table and float32 geometry."""
    import numpy as np
    import torch

    from smart_tree_amd.data_types.branch import BranchSkeleton
    from smart_tree_amd.data_types.tree import DisjointTreeSkeleton, TreeSkeleton

    g = torch.Generator().manual_seed(0)
    xyz = [torch.rand((n, 3), generator=g) for n in (4, 3, 5)]
    rad = [torch.rand((n, 1), generator=g) for n in (4, 3, 5)]
    sk = DisjointTreeSkeleton([TreeSkeleton(0, {0: BranchSkeleton(0, -1, xyz[0], rad[0]), 1: BranchSkeleton(1, 0, xyz[1], rad[1])}),
                               TreeSkeleton(1, {0: BranchSkeleton(0, -1, xyz[2], rad[2])})])
    shapes = bench.dump_outputs(sk, tmp_path / "out")
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert shapes == {k: list(v.shape) for k, v in got.items()}
    assert got["skeleton_branches"].dtype == np.float64 and got["skeleton_xyz"].dtype == np.float32
    np.testing.assert_array_equal(got["skeleton_branches"], [[0, 0, -1, 0, 4], [0, 1, 0, 4, 3], [1, 0, -1, 7, 5]])
    np.testing.assert_array_equal(got["skeleton_xyz"], torch.cat(xyz).numpy())
    np.testing.assert_array_equal(got["skeleton_radius"], torch.cat(rad).reshape(-1).numpy())


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_strong_scaling_split_of_configs2(world):
    """--scaling strong --clouds 64: the fixed batch of 64 seeds is dealt round-robin; every seed runs on exactly one rank and the
    ranks' shares differ by at most one cloud (configs[2]: 8 clouds on each of 8 GPUs)."""
    from smart_tree_amd.sharding import shard_indices

    shares = [shard_indices(64, r, world) for r in range(world)]
    assert sorted(s for sh in shares for s in sh) == list(range(64))
    assert max(map(len, shares)) - min(map(len, shares)) <= 1
    assert all(len(sh) == 64 // world for sh in shares)
