"""The designs of tests/solve_sequence_cases.py, pinned on the oracle (no device): the fields hold the tiles and closed tiles
they are built for, every step is what its sequence needs it to be, and a solver that hands the closed tiles the warm start's
residual in place of the right-hand side (wrong_warm_closed) cannot pass the bar of tests/test_gpu_solve_sequences.py."""
import numpy as np
import pytest

from tests import solve_sequence_cases as q

ALL = list(q.SEQUENCES) + ["hot_A", "hot_S"]


def steps_of(name):
    return list(zip(range(100), q.fields_of(name), q.records(name)))


@pytest.mark.parametrize("field", q.FIELDS)
def test_fields_hold_the_tiles_they_are_built_for(field):
    rec = q.solved(q.Step(field))
    assert len(rec["tiles"]) == q.TILES[field]
    if field == "A":
        assert rec["closed"] == q.CLOSED_A
        assert rec["tiles"][(3, 1, 1)] == 64
    elif field == "B":
        assert (0, 1, 0) not in rec["tiles"]
        assert rec["tiles"][(3, 1, 1)] == 65 and (3, 1, 1) not in rec["closed"]
        assert rec["closed"] == q.CLOSED_A - {(0, 1, 0), (3, 1, 1)}
        n_new = int((np.floor(q.particles("B")["pos"]).astype(int) == np.array(q.B_EXTRA_CELL)).all(axis=1).sum())
        assert 1 <= n_new <= 3
    else:
        assert rec["closed"] == set(rec["tiles"]) == q.CLOSED_A  # nothing for the PCG to iterate over
    assert set(q.group_indices(field, rec)) == set(q.groups(field))


@pytest.mark.parametrize("name", ALL)
def test_every_step_is_what_its_sequence_needs(name):
    """f = 0: a right-hand side the early-out takes, and the oracle's p = 0 in 0 iterations. NaN: b is NaN in the intended tile and
    nowhere else. Every other step is well-posed: the oracle converges, p is finite and no group's pressures are noise."""
    for k, field, rec in steps_of(name):
        step = None if name.startswith("hot_") else q.SEQUENCES[name][k]
        assert len(rec["fluid_cells"]) == len(rec["b"]) == len(rec["abits"])
        if step is not None and step.nan is not None:
            bad = np.isnan(rec["b"])
            assert bad.any() and np.isfinite(rec["b"][~bad]).all()
            assert {tuple(int(a) for a in t) for t in q.tile_of_unknowns(rec)[bad]} == {q.NAN_TILE[field]}
            assert q.NAN_TILE[field] in rec["tiles"] and (q.NAN_TILE[field] in rec["closed"]) == (field == "S")
            continue
        if step is not None and step.f == 0.0:
            assert float((rec["b"] ** 2).sum()) < 1e-6
            assert rec["iters"] == 0 and not rec["p"].any()
            continue
        assert float((rec["b"] ** 2).sum()) >= 1.0
        assert rec["residual"] < 1e-6 and 0 < rec["iters"] < 200
        assert np.isfinite(rec["p"]).all()
        for g, at in q.group_indices(field, rec).items():
            assert np.abs(rec["p"][at]).max() >= 1.0, (name, k, g)


@pytest.mark.parametrize("field", ["A", "S"])
def test_staged_hot_steps_are_the_oracles_hot_step(field):
    o = q._oracle(field)
    for rec in q.hot_steps(field):
        p, res, it = o.hot_step(q.DT)
        assert np.array_equal(p, rec["p"]) and it == rec["iters"]
        assert np.array_equal(o.cells()["vel"], rec["grid_vel"])
    o.close()


def test_step_of_the_same_system_is_the_same_record():
    assert q.solved(q.SEQUENCES["repeat"][0]) is q.solved(q.SEQUENCES["repeat"][1])
    a, c = q.solved(q.Step("A")), q.solved(q.Step("A", 1.001))
    assert np.array_equal(a["abits"], c["abits"]) and not np.array_equal(a["b"], c["b"])


@pytest.mark.parametrize("name", q.WARM_DISCRIMINATING)
def test_the_warm_start_mistake_on_closed_tiles_cannot_pass(name):
    """Every warm step (all but the first) of `repeat`, `come_and_go` and `hot`: the pressure with the mistake misses the group bar
    of the GPU test - P_REL of the group's own largest pressure - by more than 10 x on at least one closed group.

    That the comparison has to be group by group could NOT be shown by a step on which the mistake stays inside the whole-field bar
    P_REL max|p|: the previous pressure of a droplet (5 .. 400) is no small number beside that bar (0.23 on A, 0.04 on S); the
    smallest whole-field miss is 1 700 x, against 8 800 x .. 123 000 x group by group. The property is dropped; what the groups add is
    the factor between the two (and the cold test's finding that `in_solid` is the worst group at 0.014 of its bar while the whole field
    sits at 0.002)."""
    recs, fields = q.records(name), q.fields_of(name)
    for k in range(1, len(recs)):
        wrong = q.wrong_warm_closed(recs[k], recs[k - 1])
        cg = q.closed_groups(fields[k], recs[k])
        assert cg
        miss = {g: float(np.abs(wrong[at] - recs[k]["p"][at]).max() / (q.P_REL * np.abs(recs[k]["p"][at]).max())) for g, at in cg.items()}
        assert max(miss.values()) > 10.0, (name, k, miss)
        # and only the closed tiles that took part in the step before carry it
        t = q.tile_of_unknowns(recs[k])
        touched = {tuple(int(a) for a in x) for x in t[wrong != recs[k]["p"]]}
        assert touched <= recs[k]["closed"] & set(recs[k - 1]["tiles"])
    if name == "come_and_go":  # tile (0,1,0) was away in step 1 (B): cold in step 2, mistake or not
        wrong = q.wrong_warm_closed(recs[2], recs[1])
        for g in ("interior", "cell7"):
            at = q.group_indices("A", recs[2])[g]
            assert np.array_equal(wrong[at], recs[2]["p"][at])
