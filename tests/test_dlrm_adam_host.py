"""DLRM with Adam, host side (CPU): the flags, the learning-rate / gradient-scaling plan and the refusals."""
import pytest

from deeplearningexamples_amd.dlrm.engine import optimizer_plan
from deeplearningexamples_amd.dlrm.main import parse_flags


def _reference_plan(lr, world, adam_emb, adam_mlp):
    """Recommendation/DLRM/dlrm/scripts/main.py:444-452 (learning rates) and :596-608, 720-730 (scale_MLP_gradients divides
    the bottom MLP's gradients -- param_groups[1:], the top MLP is skipped -- and scale_embeddings_gradients the tables', by
    world_size, under Adam only), restated."""
    emb_lr = lr if adam_emb else lr / world
    mlp_mp_lr = lr if adam_mlp else lr / world
    return {"embeddings": (emb_lr, world if adam_emb else 1), "bottom_mlp": (mlp_mp_lr, world if adam_mlp else 1),
            "top_mlp": (lr, 1)}


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("adam_emb", [False, True])
@pytest.mark.parametrize("adam_mlp", [False, True])
def test_plan_matches_reference(world, adam_emb, adam_mlp):
    got = optimizer_plan(24.0, world, adam_emb, adam_mlp)
    want = _reference_plan(24.0, world, adam_emb, adam_mlp)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k][0] == pytest.approx(want[k][0], rel=0, abs=0) and got[k][1] == want[k][1], k


def test_adam_flags_parse_and_reach_the_trainer(monkeypatch):
    f = parse_flags(["--dataset_type", "synthetic_gpu", "--Adam_embedding_optimizer", "--Adam_MLP_optimizer", "--lr", "0.001"])
    assert f.Adam_embedding_optimizer and f.Adam_MLP_optimizer and f.lr == 0.001
    f = parse_flags(["--dataset_type", "synthetic_gpu", "--Adam_embedding_optimizer=False", "--Adam_MLP_optimizer=True"])
    assert not f.Adam_embedding_optimizer and f.Adam_MLP_optimizer
    f = parse_flags(["--dataset_type", "synthetic_gpu"])
    assert not f.Adam_embedding_optimizer and not f.Adam_MLP_optimizer and f.lr == 24.0

    # main() hands both flags to DlrmTrainer: stop right at its constructor
    import deeplearningexamples_amd.dlrm.main as M
    seen = {}

    class Stop(Exception):
        pass

    class FakeTrainer:
        def __init__(self, *a, **kw):
            seen.update(kw)
            raise Stop

    class FakeModel:
        def __init__(self, *a, **kw):
            pass

    monkeypatch.setattr(M, "DlrmTrainer", FakeTrainer)
    monkeypatch.setattr(M, "DistributedDlrm", FakeModel)
    monkeypatch.setattr(M, "init_from_env", lambda: (0, 1, 0))
    with pytest.raises(Stop):
        M.main(["--dataset_type", "synthetic_gpu", "--Adam_embedding_optimizer", "--Adam_MLP_optimizer", "--lr", "0.001",
                "--synthetic_dataset_table_sizes", "10,20", "--log_path", "/dev/null"])
    assert seen["adam_embeddings"] is True and seen["adam_mlps"] is True


@pytest.mark.parametrize("flag", ["--Adam_embedding_optimizer", "--Adam_MLP_optimizer"])
def test_row_sharding_with_adam_is_refused(flag):
    with pytest.raises(SystemExit, match="table-wise"):
        parse_flags(["--dataset_type", "synthetic_gpu", "--embedding_sharding", "row", flag])
    parse_flags(["--dataset_type", "synthetic_gpu", "--embedding_sharding", "row"])          # SGD stays accepted


def test_cat_interaction_still_refused():
    with pytest.raises(SystemExit):
        parse_flags(["--dataset_type", "synthetic_gpu", "--Adam_embedding_optimizer", "--interaction_op=cat"])
