"""CPU-only: the library, the header and the binding carry sbr_cluster_evaluate under ABI 11; the test CLI's run_tests hands a cluster
model to its native evaluator; and RNNCluster's validation assembles its nine metrics from the records of one ClusterHead.evaluate
call to the very values the per-user loop computes from the same ids."""
import argparse
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sbr_rnn.h")


def test_library_header_and_binding_carry_the_call_under_abi_11():
    import sbr_amd.engine as E
    lib = E.load_library()
    assert lib.sbr_abi_version() == 11 == E.SBR_ABI_VERSION
    header = open(HEADER).read()
    assert re.search(r"#define SBR_ABI_VERSION 11\b", header)
    assert "sbr_cluster_evaluate" in E.EXPORTS and hasattr(lib, "sbr_cluster_evaluate")
    decl = re.search(r"\bint sbr_cluster_evaluate\s*\(([^;]*)\);", header).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == 13 == len(lib.sbr_cluster_evaluate.argtypes)
    for name, value in (("SBR_CEVAL_LISTS", E.CEVAL_LISTS), ("SBR_CEVAL_PRODUCT", E.CEVAL_PRODUCT)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, header).group(1)) == value
    assert E.CEVAL_LISTS != E.CEVAL_PRODUCT
    struct = re.search(r"typedef struct sbr_eval_out \{(.*?)\} sbr_eval_out;", header, flags=re.S).group(1)
    fields = re.findall(r"\b(?:u?int32_t)\s*\*\s*(\w+)\s*;", struct)
    assert fields == ["ids", "n_pred", "hits", "first_hit", "hitmask", "item_hits"] == [f[0] for f in E.SbrEvalOut._fields_]
    assert all(f[1] is ctypes.c_void_p for f in E.SbrEvalOut._fields_)
    assert ctypes.sizeof(E.SbrEvalOut) == 6 * ctypes.sizeof(ctypes.c_void_p)


class RecordingLib(object):
    """stands in for the library below ClusterHead.evaluate: records the call, fills the outputs it is handed"""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def sbr_cluster_evaluate(self, c, h, d, users, n, k, road, mode, whole, inside, cluster, size, use):
        self.calls.append(dict(c=c, h=h, d=d, n=n, k=k, road=road, mode=mode, whole=whole is not None, size=size is not None))
        if self.status == 0:
            ctypes.memset(cluster.value, 0, 4 * n)
            rec = inside._obj
            (ctypes.c_int32 * n).from_address(rec.n_pred)[:] = [k] * n
        return self.status

    def sbr_last_error(self):
        return b"k outside"


def test_the_cluster_head_counts_its_own_evaluations():
    """ClusterHead.evaluate on a stand-in library: every call is counted on the head and none on the engine, the arguments arrive in
    the C-ABI's order, the records are shaped by k and the wishes, and the engine's status mapping raises"""
    import contextlib
    import types
    from sbr_amd.engine import CEVAL_LISTS, CEVAL_PRODUCT, EVAL_EXCL_VIEWED, EVAL_EXCL_WINDOW, ClusterHead, RNNEngine
    from sbr_amd.models import RNNCluster
    assert RNNCluster.native_eval is False          # RNNEngine.evaluate still does not rank what a cluster model ranks
    assert RNNCluster.native_evaluator is not RNNCluster.__mro__[1].native_evaluator
    lib = RecordingLib()
    eng = types.SimpleNamespace(h=11, device="cpu", evaluate_calls=0, _rank_local_flush=lambda what: None, lib=lib)
    eng._check = lambda rc: RNNEngine._check(eng, rc)
    head = ClusterHead.__new__(ClusterHead)
    head.engine, head.lib, head.h, head.n_items, head.n_clusters, head.evaluate_calls = eng, lib, 22, 50, 3, 0
    head.torch = types.SimpleNamespace(cuda=types.SimpleNamespace(device=lambda dev: contextlib.nullcontext()))
    ds = types.SimpleNamespace(d=33)
    out = head.evaluate(ds, [4, 2, 7], 40, CEVAL_LISTS, EVAL_EXCL_VIEWED, want_ids=True)
    assert head.evaluate_calls == 1 and eng.evaluate_calls == 0
    assert lib.calls[-1] == dict(c=22, h=11, d=33, n=3, k=40, road=CEVAL_LISTS, mode=EVAL_EXCL_VIEWED, whole=False, size=True)
    assert out["whole"] is None and out["size"].shape == (3,) and out["cluster_use"].shape == (3,) and out["cluster"].tolist() == [0, 0, 0]
    assert out["inside"]["ids"].shape == (3, 40) and out["inside"]["hitmask"].shape == (3, 2) and out["inside"]["n_pred"].tolist() == [40] * 3
    out = head.evaluate(ds, [4, 2], 10, CEVAL_PRODUCT, EVAL_EXCL_WINDOW, want_mask=False, want_whole=True)
    assert head.evaluate_calls == 2 and eng.evaluate_calls == 0
    assert lib.calls[-1] == dict(c=22, h=11, d=33, n=2, k=10, road=CEVAL_PRODUCT, mode=EVAL_EXCL_WINDOW, whole=True, size=False)
    assert out["size"] is None and out["inside"]["ids"] is None and out["whole"]["hitmask"] is None and out["whole"]["item_hits"].shape == (50,)
    for k in (0, 51):                               # refused before the arrays are sized by k: no call, nothing counted
        try:
            head.evaluate(ds, [1], k, CEVAL_LISTS, EVAL_EXCL_VIEWED)
            raise AssertionError("k=%d accepted" % k)
        except ValueError:
            pass
    assert head.evaluate_calls == 2 and len(lib.calls) == 2
    head.lib = eng.lib = RecordingLib(status=-1)    # SBR_EINVAL from the library: the engine's mapping, and the call was counted
    try:
        head.evaluate(ds, [1], 5, CEVAL_LISTS, 3)
        raise AssertionError("SBR_EINVAL not raised")
    except ValueError:
        pass
    assert head.evaluate_calls == 3


# ------------------------------------------------------------------ run_tests routing
class FakeNativeClusterPredictor(object):
    batched_top_k = True
    batch_size, max_length, interactions_are_unique = 4, 3, True

    def __init__(self, answer):
        self.engine = object()
        self.native_calls, self.batch_calls, self.single_calls, self.answer = [], [], [], answer

    def load(self, f):
        pass

    def native_evaluator(self, dataset, which, k, mode, want_ids=False):
        self.native_calls.append((which, k, mode, want_ids))
        return self.answer

    def top_k_batch(self, sequences, user_ids=None, k=10, exclude=None):
        self.batch_calls.append(len(sequences))
        return [([0], 7) for _ in sequences]

    def top_k_recommendations(self, sequence, user_id=None, k=10, exclude=None):
        self.single_calls.append(user_id)
        return [0], 7


class FakeTestDataset(object):
    n_items = 40
    item_popularity = np.ones(40)

    def test_set(self, epochs=1):
        for u in range(6):
            yield [[u, 1.0], [u + 1, 1.0], [u + 2, 1.0], [u + 3, 1.0]], u


def test_run_tests_hands_a_cluster_model_to_its_native_evaluator():
    from sbr_amd import test as Te
    from sbr_amd.engine import EVAL_EXCL_VIEWED
    marker = argparse.Namespace(nb_of_dp=12.5)
    predictor = FakeNativeClusterPredictor(marker)
    ev = Te.run_tests(predictor, "f", FakeTestDataset(), argparse.Namespace(clusters=4), k=10)
    assert ev is marker and ev.nb_of_dp == 12.5                      # the mean cluster size the evaluator came with, not n_items
    assert predictor.native_calls == [("test", 10, EVAL_EXCL_VIEWED, True)]
    assert predictor.batch_calls == [] and predictor.single_calls == []
    # --save_rank stays on the host road, one user per call
    predictor = FakeNativeClusterPredictor(marker)
    Te.run_tests(predictor, "f", FakeTestDataset(), argparse.Namespace(clusters=4), get_full_recommendation_list=True, k=10)
    assert predictor.native_calls == [] and predictor.batch_calls == [] and predictor.single_calls == list(range(6))
    # an evaluator that declines (None) leaves the users to top_k_batch
    predictor = FakeNativeClusterPredictor(None)
    ev = Te.run_tests(predictor, "f", FakeTestDataset(), argparse.Namespace(clusters=4), k=10)
    assert len(predictor.native_calls) == 1 and predictor.batch_calls == [4, 2] and ev.nb_of_dp == 7


# ------------------------------------------------------------------ the validation's metric assembly
N_ITEMS, N_CLUSTERS, K = 60, 3, 10


class FakeSet(object):
    shuffle = False

    def __call__(self, epochs=1):
        return iter(())


class FakeDeviceSet(object):
    def __init__(self, seqs):
        self.items = np.concatenate(seqs).astype(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


class FakeValidationDataset(object):
    n_items = N_ITEMS
    item_popularity = np.ones(N_ITEMS)
    validation_set = FakeSet()

    def __init__(self, seqs):
        self.ds = FakeDeviceSet(seqs)

    def device_set(self, which, engine, ratings=False):
        assert which == "validation"
        return self.ds


def records(ids, goals):
    n = len(goals)
    rec = dict(n_pred=np.zeros(n, np.int32), hits=np.zeros(n, np.int32), first_hit=np.zeros(n, np.int32),
               hitmask=np.zeros((n, 1), np.uint32), item_hits=np.zeros(N_ITEMS, np.int32), ids=None)
    for r, g in enumerate(goals):
        rec["n_pred"][r] = len(ids[r])
        correct = set(g) & set(ids[r].tolist())
        rec["hits"][r] = len(correct)
        rec["first_hit"][r] = int(g[0] in ids[r])
        for p, i in enumerate(ids[r]):
            if i in g:
                rec["hitmask"][r, 0] |= np.uint32(1 << p)
        for i in correct:
            rec["item_hits"][i] += 1
    return rec


class FakeHead(object):
    def __init__(self, R, hard, out):
        self.R, self.hard, self.out, self.calls = R, hard, out, []

    def get_params(self):
        return self.R, None

    def hard_clusters(self):
        return self.hard

    def evaluate(self, dataset, users, k, road, exclude_mode, want_ids=False, want_mask=True, want_whole=False):
        self.calls.append((list(users), k, road, exclude_mode, want_ids, want_mask, want_whole))
        return self.out


def make_model(cluster_type, seqs, ids_whole, ids_inside, cluster, R, hard):
    from sbr_amd.models import RNNCluster
    users = [u for u, s in enumerate(seqs) if len(s) >= 2]
    goals = {u: [int(i) for i in seqs[u][len(seqs[u]) // 2:]] for u in users}

    class Model(RNNCluster):
        """the host loop's two seams answer from the same ids the records were made of"""

        def _gen_mini_batch(self, generator, test=False):
            for u in users:
                yield u, goals[u]

        def test_function(self, u):
            r = users.index(u)
            used = hard[:, np.array([cluster[r]])].T
            return ids_whole[r], ids_inside[r], int(cluster[r]), float(used[0].sum())
    m = Model.__new__(Model)
    m.n_clusters, m.n_items, m.cluster_type, m.interactions_are_unique, m.use_ratings_features = N_CLUSTERS, N_ITEMS, cluster_type, True, False
    m.dp, m.engine, m.target_selection = None, object(), argparse.Namespace(shuffle=False, determinist_test=True, bias=-1.0)
    m.dataset = FakeValidationDataset(seqs)
    g = [goals[u] for u in users]
    out = {"whole": records(ids_whole, g), "inside": records(ids_inside, g), "cluster": np.asarray(cluster, np.int32), "size": None,
           "cluster_use": np.bincount(cluster, minlength=N_CLUSTERS).astype(np.int32)}
    m.head = FakeHead(R, hard, out)
    m.metrics = {k: None for k in ("recall", "cluster_recall", "sps", "cluster_sps", "ignored_items", "assr", "cluster_use",
                                   "cluster_use_std", "cluster_size")}
    return m, users


def test_validation_metrics_from_records_equal_the_host_loop(monkeypatch):
    from sbr_amd.engine import CEVAL_PRODUCT, EVAL_EXCL_WINDOW
    rng = np.random.default_rng(0)
    seqs = [rng.integers(0, N_ITEMS, size=L) for L in (2, 7, 1, 12, 30, 5, 9, 3, 16)]      # user 2 (one item) is no validation user
    n = 8
    for cluster_type in ("mix", "softmax", "sigmoid"):
        R = rng.normal(0, 0.02, size=(N_ITEMS, N_CLUSTERS)).astype(np.float32)
        hard = (1.0 / (1.0 + np.exp(-100.0 * R))).astype(np.float32)                       # fractional memberships: sums that round
        cluster = rng.integers(0, N_CLUSTERS, size=n)
        cluster[:2] = 1                                                                    # one cluster drawn more than once; maybe one never
        ids_whole = [rng.permutation(N_ITEMS)[:K].astype(np.int32) for _ in range(n)]
        ids_inside = [rng.permutation(N_ITEMS)[:K].astype(np.int32) for _ in range(n)]
        for r, u in enumerate([0, 1, 3, 4]):                                               # some hits, the first goal item among them
            goal = seqs[u][len(seqs[u]) // 2:]
            ids_whole[r][3] = goal[0]; ids_inside[r][7] = goal[-1]
        m, users = make_model(cluster_type, seqs, ids_whole, ids_inside, cluster, R, hard)
        assert users == [0, 1, 3, 4, 5, 6, 7, 8]
        monkeypatch.setenv("SBR_NATIVE_EVAL", "1")
        new = m._compute_validation_metrics({k: [] for k in m.metrics})
        assert m.head.calls == [(users, K, CEVAL_PRODUCT, EVAL_EXCL_WINDOW, False, True, True)]
        monkeypatch.setenv("SBR_NATIVE_EVAL", "0")
        old = m._compute_validation_metrics({k: [] for k in m.metrics})
        assert len(m.head.calls) == 1
        assert set(new) == set(old) and len(old) == 9
        for name in old:
            a, b = new[name][0], old[name][0]
            if name in ("cluster_use", "cluster_size"):
                assert np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b), name
            else:
                assert a == b and type(a) is type(b), (name, a, b)
        assert old["recall"][0] > 0 and old["sps"][0] > 0 and old["assr"][0] > 1
