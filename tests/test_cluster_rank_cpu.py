"""CPU-only: the library, the header and the binding carry sbr_cluster_lists / sbr_cluster_rank under ABI 11, RNNCluster offers the
batched ranking, and the test CLI's run_tests sends a cluster model's users through it (test.py:61-76: ranked inside the user's
cluster, nb_of_dp = the mean number of items scored)."""
import argparse
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_and_header_carry_the_two_calls_under_abi_11():
    import sbr_amd.engine as E
    lib = E.load_library()
    assert lib.sbr_abi_version() == 11 == E.SBR_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "sbr_rnn.h")).read()
    assert re.search(r"#define SBR_ABI_VERSION 11\b", header)
    for name, n_args in (("sbr_cluster_lists", 3), ("sbr_cluster_rank", 10)):
        assert name in E.EXPORTS
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == n_args
        assert re.search(r"\bint %s\s*\(" % name, header)
    assert "added under ABI 11" in header


def test_the_switch_is_read_with_the_others():
    src = open(os.path.join(ROOT, "sequence-based-recommendations_amd", "csrc", "sbr_api.hip")).read()
    body = src[src.index("static SbrSwitches sbr_read_switches()"):]
    body = body[:body.index("return sw;")]
    assert '"SBR_CLUSTER_RANK"' in body
    assert src.count("getenv(") == body.count("getenv(")              # still the library's only reads of the environment


def test_rnncluster_offers_the_batched_ranking():
    from sbr_amd.models import RNNCluster
    assert RNNCluster.batched_top_k is True
    assert "NotImplementedError" not in RNNCluster.top_k_batch.__doc__


class FakeEngine(object):
    """what run_tests asks of an engine before it batches: a rank attribute; the whole-catalogue test function must stay unused"""

    def rank(self, *a, **kw):
        raise AssertionError("a cluster model is never ranked over the whole catalogue")

    def test_function(self, *a, **kw):
        raise AssertionError("a cluster model's users never go through engine.test_function")


class FakeClusterPredictor(object):
    """a stand-in cluster predictor: top_k_batch records its calls and answers (ids, n) per sequence"""
    batched_top_k = True
    batch_size, max_length, interactions_are_unique = 4, 3, True

    def __init__(self, n_items):
        self.engine = FakeEngine()
        self.n_items = n_items
        self.batch_calls, self.single_calls, self.loaded = [], [], []

    def load(self, f):
        self.loaded.append(f)

    def _answer(self, seq, k):
        seen = {x[0] for x in seq}
        first = (seq[-1][0] + 1) if seq else 0
        ids = [i % self.n_items for i in range(first, first + self.n_items) if i % self.n_items not in seen][:k]
        return ids, 10 + (first % 7)                                  # a cluster "size" that differs from user to user

    def top_k_batch(self, sequences, user_ids=None, k=10, exclude=None):
        assert 1 <= len(sequences) <= self.batch_size and all(len(s) for s in sequences)
        self.batch_calls.append(([list(s) for s in sequences], list(user_ids), k))
        return [self._answer(s, k) for s in sequences]

    def top_k_recommendations(self, sequence, user_id=None, k=10, exclude=None):
        self.single_calls.append((list(sequence), user_id, k))
        return self._answer(sequence, k)


class FakeDataset(object):
    def __init__(self, n_items, sequences):
        self.n_items = n_items
        self.item_popularity = np.ones(n_items)
        self.sequences = sequences

    def test_set(self, epochs=1):
        for u, s in enumerate(self.sequences):
            yield s, u


def sequences_for(n_items):
    rng = np.random.default_rng(0)
    seqs = []
    for u in range(11):
        n = int(rng.integers(2, 12))                                  # viewed halves of 1 .. 5 items: shorter and longer than the window of 3
        seqs.append([[int(i), 1.0] for i in rng.permutation(n_items)[:n]])
    seqs.append([[5, 1.0]])                                           # a sequence of one item: an empty viewed half
    return seqs


def test_run_tests_routes_a_cluster_model_through_top_k_batch():
    from sbr_amd import test as Te
    from sbr_amd.data import Evaluator
    n_items = 40
    seqs = sequences_for(n_items)
    for k in (10, 30):                                               # k above the engine's 64 is the same road: see the GPU file for k = 100
        dataset = FakeDataset(n_items, seqs)
        predictor = FakeClusterPredictor(n_items)
        ev = Te.run_tests(predictor, "some_file", dataset, argparse.Namespace(clusters=4), k=k)
        assert predictor.loaded == ["some_file"]
        # every user with a viewed half went through top_k_batch, batch_size at a time, in order, whatever k and the length
        sent = [s for call in predictor.batch_calls for s in call[0]]
        assert sent == [s[:len(s) // 2] for s in seqs if len(s) // 2 > 0]
        assert [len(c[0]) for c in predictor.batch_calls] == [4, 4, 3]
        assert all(c[2] == k for c in predictor.batch_calls)
        assert [u for c in predictor.batch_calls for u in c[1]] == list(range(11))
        # the empty viewed half stays per user, and its tuple is unpacked
        assert predictor.single_calls == [([], 11, k)]
        expected = Evaluator(dataset, k=k)
        ns = []
        for s in seqs:
            ids, n = predictor._answer(s[:len(s) // 2], k)
            expected.add_instance([i[0] for i in s[len(s) // 2:]], ids)
            ns.append(n)
        for m in ("sps", "recall", "precision", "ndcg", "item_coverage", "user_coverage"):
            assert ev.metrics[m]() == expected.metrics[m](), m
        assert ev.nb_of_dp == np.mean(ns) and ev.nb_of_dp < n_items
        assert len(set(ns)) > 1


def test_run_tests_save_rank_stays_per_user_and_unpacks_the_tuple():
    from sbr_amd import test as Te
    n_items = 40
    seqs = sequences_for(n_items)
    predictor = FakeClusterPredictor(n_items)
    ev = Te.run_tests(predictor, "f", FakeDataset(n_items, seqs), argparse.Namespace(clusters=4), get_full_recommendation_list=True, k=10)
    assert predictor.batch_calls == []
    assert [c[2] for c in predictor.single_calls] == [n_items] * len(seqs)
    assert ev.nb_of_dp == np.mean([predictor._answer(s[:len(s) // 2], n_items)[1] for s in seqs])
    for (goal, predicted), s in zip(ev.instances, seqs):             # ids, not the (ids, n) pair as a two-element list
        assert predicted == predictor._answer(s[:len(s) // 2], n_items)[0]
