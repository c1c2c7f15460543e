"""
GeneticTraining without an engine: the parent blocks of the next generation
(the reference's array_split lengths, genetic_algorithm.py:107-108, 256-264),
the parent selection (best first, then a reproducible draw without
replacement from all ids, :291-302) and the argument checks.
"""

import types

import numpy as np
import pytest

from swarmrl_amd.training_routines import GeneticTraining


def _routine(tmp_path, population, parents, **kwargs):
    trainer = types.SimpleNamespace(n_members=population, agents={})
    return GeneticTraining(trainer, lambda: None, population_size=population,
                           number_of_parents=parents, output_directory=tmp_path, **kwargs)


@pytest.mark.parametrize("population, parents, lengths",
                         [(10, 2, [5, 5]), (10, 3, [4, 3, 3]), (4, 1, [4])])
def test_parent_of_follows_the_reference_block_lengths(tmp_path, population, parents, lengths):
    routine = _routine(tmp_path, population, parents)
    assert routine.split_lengths == lengths
    ids = list(range(7, 7 - parents, -1))  # parents 7, 6, ...: any ids, in this order
    parent_of = routine._parent_of(ids)
    assert len(parent_of) == population
    expected = [i for i, n in zip(ids, lengths) for _ in range(n)]
    assert parent_of == expected


def test_select_parents_puts_the_best_first_and_is_reproducible(tmp_path):
    scores = np.array([0.5, -1.0, 3.5, 3.0, 0.0, 2.0])
    a = _routine(tmp_path / "a", 6, 3, rng=11)
    b = _routine(tmp_path / "b", 6, 3, rng=11)
    draws_a = [a._select_parents(scores) for _ in range(5)]
    draws_b = [b._select_parents(scores) for _ in range(5)]
    assert draws_a == draws_b
    for parents, reward in draws_a:
        assert parents[0] == 2 and reward == 3.5 and len(parents) == 3
        assert len(set(parents[1:])) == 2 and all(0 <= i < 6 for i in parents)
    # the draw is numpy.random.default_rng(rng).choice without replacement
    rng = np.random.default_rng(11)
    assert draws_a[0][0][1:] == list(rng.choice(list(range(6)), size=2, replace=False))
    other = _routine(tmp_path / "c", 6, 3, rng=12)
    assert [other._select_parents(scores) for _ in range(5)] != draws_a
    assert _routine(tmp_path / "d", 6, 1)._select_parents(scores) == ([2], 3.5)


def test_scores_reduce_the_whole_history(tmp_path):
    history = np.array([0.0, 1.0, 4.0])
    for method, want in (("sum", 5.0), ("mean", 5.0 / 3.0), ("max", 4.0)):
        routine = _routine(tmp_path / method, 2, 1, parent_selection_method=method)
        assert routine._select_fn(history) == pytest.approx(want)


def test_bad_arguments_raise(tmp_path):
    with pytest.raises(ValueError):
        _routine(tmp_path, 4, 2, parent_selection_method="median")
    with pytest.raises(ValueError):
        _routine(tmp_path, 4, 2, cluster=object())
    trainer = types.SimpleNamespace(n_members=3, agents={})
    with pytest.raises(ValueError):
        GeneticTraining(trainer, lambda: None, population_size=4, output_directory=tmp_path)
    routine = _routine(tmp_path, 4, 2, parallel_jobs=9)  # accepted and ignored
    assert (tmp_path / "genetic_algorithm").is_dir() and routine.parallel_jobs == 9
