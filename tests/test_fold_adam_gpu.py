"""tn_train_step with the main grid's fold stepping its own table (the default) against the same iterations with TN_FOLD_ADAM=0 (the fold stores
the table gradient, the Adam launch steps the table): same training state, skip counts, loss scale and schedule lag after every iteration, the
gradient arena left zero, and the device-side decision word saying which path ran.  The library reads the switch once per process, so the
unfused runs come from ONE worker process for all cases (tests/fold_adam_worker.py); the cases themselves are in tests/fold_adam_cases.py."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import GOLDEN_RAYS
from fold_adam_cases import FELL_BACK, FUSED, NONE, POISON, guard_limit, run_case, seeded_mask
from test_trainer_sequence_gpu import assert_same_training_state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def unfused(golden_dir, tmp_path_factory):
    assert os.environ.get("TN_FOLD_ADAM", "1") != "0", "this process runs the default path; the worker runs TN_FOLD_ADAM=0"
    out = str(tmp_path_factory.mktemp("fold_adam") / "unfused.pt")
    p = subprocess.run([sys.executable, os.path.join(HERE, "fold_adam_worker.py"), golden_dir, out], env=dict(os.environ, TN_FOLD_ADAM="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return torch.load(out, weights_only=False)


def _same_iterations(name, F, U):
    assert len(F) == len(U)
    for i, (f, u) in enumerate(zip(F, U)):
        assert_same_training_state(f["state"], u["state"], f"{name}: fold-side Adam vs TN_FOLD_ADAM=0, iteration {i}")
        assert (f["scale"], f["lag"], f["skipped"]) == (u["scale"], u["lag"], u["skipped"]), (name, i)
        assert (f["updated"], f["counters"]) == (u["updated"], u["counters"]), (name, i)
        assert f["grads_max"] == 0.0 and u["grads_max"] == 0.0, (name, i)  # the arena stays zero: what table_grad_is_zero promises the next iteration
        assert u["decision"] == NONE, (name, i)  # (the switch took: the worker's fold was never armed)


@pytest.mark.parametrize("name", ["seq12", "seq13"])
def test_thirteen_iterations_with_a_forced_inf(golden_dir, unfused, name):
    """Iterations with and without a proposal update (the schedule thins out after the first ten) and an inf image at iteration 6: the inf reaches
    d enc, so that iteration falls back and is skipped by the unfused launches; every other one is stepped by the fold."""
    U = unfused[name]
    F = run_case(name, golden_dir, ref=U)
    _same_iterations(name, F, U)
    assert [f["decision"] for f in F] == [FELL_BACK if i == 6 else FUSED for i in range(13)]
    assert any(f["updated"] for f in F) and not all(f["updated"] for f in F)
    assert F[-1]["scale"] == 32768.0 and F[-1]["lag"] == 1 and sum(F[-1]["skipped"]) == 2  # (fields and camera_opt skipped once)


def test_bucket_without_records_decays_its_moments(golden_dir, unfused):
    """One 2 x 2 patch of rays on a 2^18 table: most of level 0's 64 buckets receive no record.  Every second slot of the level carries moments
    from "earlier" iterations (seeded): in a bucket without records they decay and move their parameters exactly as the Adam launch does --
    bit for bit, no gradient is involved -- and the slots that carry nothing keep parameters and moments bit-identical."""
    (u,), (f,) = unfused["empty18"], run_case("empty18", golden_dir)
    assert f["decision"] == FUSED and f["grads_max"] == 0.0
    pre_p, pre_m, pre_v = (t.view(64, 8192) for t in f["pre"])
    up, um, uv = (t.view(64, 8192) for t in u["state"])
    fp, fm, fv = (t.view(64, 8192) for t in f["state"])
    seeded = seeded_mask(8192)
    # a bucket without records on the unfused path: nothing arrived on the unseeded slots, the seeded first moments are beta1 x what they were
    empty = ((um[:, ~seeded] == 0) & (uv[:, ~seeded] == 0)).all(1) & (um[:, seeded] == pre_m[:, seeded] * torch.tensor(0.9)).all(1)
    assert int(empty.sum()) >= 1, int(empty.sum())
    for x, y in ((fp, up), (fm, um), (fv, uv)):
        assert torch.equal(x[empty], y[empty])
    assert bool((fp[empty][:, seeded] != pre_p[empty][:, seeded]).any())  # the seeded slots moved
    assert torch.equal(fp[empty][:, ~seeded], pre_p[empty][:, ~seeded]) and not bool(fm[empty][:, ~seeded].any()) and not bool(fv[empty][:, ~seeded].any())
    assert_same_training_state(f["state"], u["state"], "level 0, every bucket")
    assert (f["scale"], f["skipped"]) == (u["scale"], u["skipped"])


def test_non_finite_in_the_small_ranges_only(golden_dir, unfused):
    """inf in the gradient of ONE element of the field's small ranges, d enc finite, on four iterations (fold_adam_cases.POISON: elements away
    from every multiple of 64 of their range, in different waves and load batches of the checking launch; iterations with a proposal update,
    where nothing in or before the fold launch but that launch can raise the flag, and without): the launch between bin and fold raises the
    group's flag before the fold starts, the fold leaves the table alone (still the fused decision), one skip is counted each time, and the
    iterations in between step again."""
    U = unfused["small_inf"]
    F = run_case("small_inf", golden_dir, ref=U)
    _same_iterations("small_inf", F, U)
    assert [f["decision"] for f in F] == [FUSED] * len(F)
    lo, hi = F[0]["table"]
    skips = 0
    for i, f in enumerate(F):
        same = [torch.equal(before[lo:hi], after[lo:hi]) for before, after in zip(f["pre"], f["state"])]
        if i in POISON:
            skips += 1
            assert all(same), (i, same)  # parameters and both moments of the table bit-identical
        else:
            assert not same[0], i
        assert sum(f["skipped"]) == skips, (i, f["skipped"])
    assert {F[i]["updated"] for i in POISON} == {True, False}


def test_guard_trip_falls_back(golden_dir, unfused):
    """A finite batch whose max |d enc| exceeds FLT_MAX / (8 P): the fold stores the gradients and checks the final values, the Adam launch steps
    the table, as without the switch.  The image is multiplied by fold_adam_cases.GUARD_IMAGE_SCALE (the figures it was chosen from are there);
    nothing overflows, so the iteration is stepped, not skipped."""
    U = unfused["guard"]
    F = run_case("guard", golden_dir, ref=U)
    _same_iterations("guard", F, U)
    assert [f["decision"] for f in F] == [FUSED, FELL_BACK]
    assert guard_limit(GOLDEN_RAYS) < F[1]["enc_max"] < float("inf") and sum(F[1]["skipped"]) == 0


def test_more_than_one_fold_block_per_bucket_stays_unfused(golden_dir, unfused):
    """10944 rays x 48 samples = 525312 > 1024 bin blocks x 512 samples: seg_plan cuts the buckets into two chunks, no block owns a bucket, the
    host does not arm the fold (the decision word stays 0)."""
    U = unfused["chunks"]
    F = run_case("chunks", golden_dir, ref=U)
    _same_iterations("chunks", F, U)
    assert [f["decision"] for f in F] == [NONE, NONE]
