"""bench.py's command line and --dump-outputs writer, without a GPU: --steps is the number of steps of a timed region
and cannot be zero; the dump directory is resolved where bench.py is started; each rate's last timed step is written
as <rate>_params.npy / <rate>_winner.npy in float64."""
import os

import numpy as np
import pytest

import bench


def test_steps_must_be_positive():
    assert bench.parse(["--steps", "7"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_full_is_opt_in():
    """a plain run times the steps and prints the line; the analysis beside it is asked for with --full"""
    assert bench.parse([]).full is False
    assert bench.parse(["--full"]).full is True


def test_dump_directory_is_absolute_and_off_by_default(tmp_path, monkeypatch):
    assert bench.parse([]).dump_outputs is None
    monkeypatch.chdir(tmp_path)
    assert bench.parse(["--dump-outputs", "out"]).dump_outputs == os.path.join(str(tmp_path), "out")


def test_dump_outputs_files(tmp_path):
    last = {"votes": 5001, "index": 17, "fit": np.array([0.1, -0.2, 0.97, 1.5, 2.5, -3.5]), "cnt": 5003,
            "lm_info": 0, "lm_nfev": 0, "cost": 0.0, "lm_stall": 0}
    bench.dump_outputs(str(tmp_path / "d"), [("full_count", last), ("early_exit", None)])
    assert sorted(os.listdir(tmp_path / "d")) == ["early_exit_params.npy", "early_exit_winner.npy",
                                                  "full_count_params.npy", "full_count_winner.npy"]
    p = np.load(tmp_path / "d" / "full_count_params.npy")
    w = np.load(tmp_path / "d" / "full_count_winner.npy")
    assert p.dtype == w.dtype == np.float64
    assert np.array_equal(p, last["fit"]) and w.tolist() == [5001, 17, 5003, 0, 0, 0.0]
    # a rate whose last step had no winner: empty fit, zero record
    assert np.load(tmp_path / "d" / "early_exit_params.npy").shape == (0,)
    assert not np.load(tmp_path / "d" / "early_exit_winner.npy").any()
