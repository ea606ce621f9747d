"""The host half of the FM trainer (tfrecomm_amd/fm.py): the five-way split of the users and the sizing of each resident step
from the store's row lengths."""
import numpy as np
import pytest

from tfrecomm_amd import fm
from tests import fm_fit_ref as FR


@pytest.mark.parametrize("n_users", [5, 23, 150])
def test_kfold_by_user_puts_every_user_in_exactly_one_test_fold(n_users):
    rs = np.random.RandomState(1)
    users = np.concatenate((rs.permutation(n_users), rs.randint(0, n_users, 400))) * 3 + 7     # every user, ids with gaps
    folds = fm.kfold_by_user(users, 5, seed=4)
    assert len(folds) == 5
    tests = np.concatenate([t for _, t in folds])
    assert sorted(tests.tolist()) == sorted(set(users.tolist()))                  # each user once
    sizes = [t.size for _, t in folds]
    assert max(sizes) - min(sizes) <= 1
    for train, test in folds:
        assert not set(train.tolist()) & set(test.tolist())
        assert sorted(np.concatenate((train, test)).tolist()) == sorted(set(users.tolist()))


def test_kfold_by_user_is_the_seeded_permutation_of_the_users_in_order_of_first_appearance():
    users = np.array([9, 2, 9, 7, 2, 4, 11, 7, 0, 5, 3])
    first = np.array([9, 2, 7, 4, 11, 0, 5, 3])
    want = np.array_split(first[np.random.RandomState(6).permutation(first.size)], 5)
    got = fm.kfold_by_user(users, 5, seed=6)
    for k in range(5):
        assert np.array_equal(got[k][1], want[k])
    again = fm.kfold_by_user(users, 5, seed=6)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, again))
    other = fm.kfold_by_user(users, 5, seed=7)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(got, other))
    with pytest.raises(ValueError):
        fm.kfold_by_user(users[:3], 5, seed=0)                                    # fewer users than folds


def test_plan_steps_is_the_entry_count_of_each_steps_rows():
    x, _ = FR.store("train")
    lengths = np.diff(x.indptr)
    ids = FR.train_ids(64)
    got = fm.plan_steps(lengths, ids, 64)
    assert got.dtype == np.int64 and got.shape == (6,)
    for s in range(6):
        assert got[s] == np.diff(x[ids[s * 64:(s + 1) * 64]].indptr).sum()
    assert got[3] == 0                                                            # the step of empty rows
    for name, b in FR.batches().items():
        assert fm.plan_steps(lengths, b, b.size)[0] == x[b].nnz, name


@pytest.mark.parametrize("bad", [-1, FR.N])
def test_plan_steps_refuses_an_id_outside_the_store(bad):
    lengths = np.diff(FR.store("train")[0].indptr)
    ids = FR.train_ids(64).copy()
    ids[200] = bad
    with pytest.raises(IndexError):
        fm.plan_steps(lengths, ids, 64)
    with pytest.raises(ValueError):
        fm.plan_steps(lengths, ids[:100], 64)                                     # not a whole number of batches


def test_driver_refuses_dimension_zero():
    df = {"user": np.array([0, 1]), "item": np.array([0, 1]), "outcome": np.array([0.0, 1.0], np.float32)}
    with pytest.raises(ValueError, match="LogisticRegression"):
        fm.run(df, 2, 2, ["users", "items"], 0, 1, 1, 0.01, 0.0, "sgd", 0)
    with pytest.raises(ValueError):
        fm.main(["--dataset", "none", "--d", "0", "--users", "--items"])
