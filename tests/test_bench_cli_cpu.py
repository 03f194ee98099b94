"""bench.py's command line and --dump-outputs writer on CPU: a plain run takes no
--part, and the dump holds float32 / float64 arrays, a large one as the same seeded
sample of positions on every call."""
import types

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("argv", [["--part", "scan"], ["--part", "train", "--steps", "2"],
                                  ["--full", "--part", "scan", "--dump-outputs", "x"]])
def test_rejected_arguments(monkeypatch, argv):
    import bench

    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2  # argparse's usage error, before any device is touched


def _fake_state(n):
    g = torch.Generator().manual_seed(3)
    head = lambda: types.SimpleNamespace(flat=torch.randn(n, generator=g))  # noqa: E731
    model = types.SimpleNamespace(encoder_q=head(), encoder_k=head(), use_momentum=True,
                                  use_queue=True, queue=torch.randn(8, 50, generator=g))
    st = types.SimpleNamespace(loss_record=[torch.tensor(0.25), torch.tensor(1.5)],
                               grad_norm=torch.tensor([2.0, 0.5, 0.0, 0.0]))
    return model, st


def test_dump_outputs(monkeypatch, tmp_path):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    model, st = _fake_state(5000)
    bench.dump_outputs(str(tmp_path / "a"), model, st)
    bench.dump_outputs(str(tmp_path / "b"), model, st)
    got = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["encoder_k_params.npy", "encoder_q_params.npy", "grad_norm.npy",
                           "loss.npy", "queue.npy"]
    assert got["loss.npy"].dtype == np.float64 and got["loss.npy"].tolist() == [1.5]
    assert got["grad_norm.npy"].dtype == np.float64 and got["grad_norm.npy"].tolist() == [2.0]
    assert np.array_equal(got["queue.npy"], model.queue.numpy())  # below the cap: whole
    idx = np.sort(np.random.default_rng(0).choice(5000, 1000, replace=False))
    for name, head in (("encoder_q_params.npy", model.encoder_q),
                       ("encoder_k_params.npy", model.encoder_k)):
        assert got[name].dtype == np.float32 and got[name].shape == (1000,)
        assert np.array_equal(got[name], head.flat.numpy()[idx])
        assert np.array_equal(got[name], np.load(tmp_path / "b" / name))
