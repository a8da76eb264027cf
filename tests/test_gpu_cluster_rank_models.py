"""RNNCluster.top_k_batch and `python -m sbr_amd.test --clusters C`: every user is ranked inside their item cluster on the device
(sbr_cluster_rank), and the test CLI reports cluster-restricted metrics with the mean cluster size (test.py:61-76).

The expected lists are exact: the raw scores of engine.predict_function, restricted to predictor.clusters[c] (prepare_tests) with
c from head.select, viewed and excluded ids dropped, ordered by np.lexsort((ids, -scores)).  The host scoring of
top_k_recommendations (a numpy dot product) rounds differently from the device, so its ids are NOT compared; its integer outputs
-- the number of items scored, and the cluster it selected -- are."""
import glob

import numpy as np
import pytest

from test_gpu_train_cli import make_dataset

pytestmark = pytest.mark.gpu

N_ITEMS = 300
BASE = ["-b", "8", "--max_length", "6", "--r_t", "GRU", "--r_l", "16", "--clusters", "4", "--sampling", "8"]
METRICS = ("sps", "recall", "ndcg", "item_coverage", "user_coverage", "blockbuster_share", "precision", "assr")


def trained_predictor(root, parser, extra=()):
    from sbr_amd import options as parse
    from sbr_amd.data import DataHandler
    args = parse.command_parser(parse.predictor_command_parser, parser, argv=["-d", root] + BASE + list(extra))
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    return predictor, dataset, args


def expected_answers(predictor, sequences, exclude, k):
    """[(ids, n, cluster)]: the exact ranking inside each user's cluster, batch_size rows per engine call"""
    out = []
    B, T = predictor.batch_size, predictor.max_length
    predictor.prepare_tests()
    for lo in range(0, len(sequences), B):
        chunk = sequences[lo:lo + B]
        X = np.zeros((len(chunk), T, 1), dtype=np.int32); mask = np.zeros((len(chunk), T), dtype=np.float32)
        for i, s in enumerate(chunk):
            w = s[-T:]
            X[i, :len(w), 0] = [x[0] for x in w]; mask[i, :len(w)] = 1
        scores = predictor.engine.predict_function(X, mask)
        csel = predictor.head.select(len(chunk))
        for i, s in enumerate(chunk):
            mem = np.asarray(predictor.clusters[int(csel[i])], dtype=np.int64)
            gone = {x[0] for x in s} | set(int(e) for e in (exclude[lo + i] or []))
            ok = ~np.isnan(scores[i, mem]) & (scores[i, mem] > -np.inf) & ~np.isin(mem, sorted(gone))
            ids = mem[ok]
            ids = ids[np.lexsort((ids, -scores[i, ids]))][:k]
            out.append(([int(j) for j in ids], len(mem), int(csel[i])))
    return out


def test_top_k_batch_ranks_inside_the_users_cluster(tmp_path):
    from sbr_amd import options as parse
    root = make_dataset(str(tmp_path / "ds"), n_users=60, n_items=N_ITEMS)
    predictor, dataset, _ = trained_predictor(root, parse.training_command_parser)
    try:
        assert predictor.batched_top_k and predictor.predict_with_clusters
        predictor.train(dataset, max_iter=20, progress=10 ** 9, autosave="None")
        sequences = [seq for seq, _ in dataset.test_set(epochs=1)] + [seq for seq, _ in dataset.validation_set(epochs=1)]
        sequences += [s[:3] for s in sequences[:4]] + [sequences[0] + sequences[1]]      # short ones, and one far longer than the window
        users = list(range(len(sequences)))
        assert len(sequences) > predictor.batch_size and max(len(s) for s in sequences) > predictor.max_length
        assert min(len(s) for s in sequences) < predictor.max_length
        exclude = [None] * len(sequences)
        exclude[2] = [1, 2, 3, 250, 250]
        exclude[9] = list(range(100, 180))
        exclude[11] = []
        for k in (5, 100):
            want = expected_answers(predictor, sequences, exclude, k)
            many = predictor.top_k_batch(sequences, user_ids=users, k=k, exclude=exclude)
            assert predictor.engine.query("cluster_rank_form") == 1
            assert len(many) == len(sequences)
            for i, ((ids, n), (wids, wn, wc)) in enumerate(zip(many, want)):
                assert ids == wids and n == wn, (i, k)
                assert all(isinstance(j, int) for j in ids) and isinstance(n, int)
                assert len(ids) == min(k, len(wids)) and n < N_ITEMS
                one_ids, one_n = predictor.top_k_recommendations(sequences[i], user_id=users[i], k=k, exclude=exclude[i])
                assert one_n == n and int(predictor.head.select(1)[0]) == wc      # the integer outputs of the host road
                assert not set(ids) & {x[0] for x in sequences[i]}    # interactions are unique: nothing viewed comes back
            assert not set(many[9][0]) & set(exclude[9]) and not set(many[2][0]) & {1, 2, 3, 250}
        assert len({c for _, _, c in want}) >= 2                      # the users do not all share one cluster
        assert predictor.top_k_batch([], k=5) == []
    finally:
        predictor.head.close(); predictor.engine.close()


def test_top_k_batch_without_clusters_is_the_whole_catalogue_road(tmp_path):
    from sbr_amd import options as parse
    from sbr_amd.models import RNNBase
    root = make_dataset(str(tmp_path / "ds"), n_users=60, n_items=N_ITEMS)
    predictor, dataset, _ = trained_predictor(root, parse.training_command_parser, extra=["--ignore_clusters"])
    try:
        assert not predictor.predict_with_clusters
        predictor.train(dataset, max_iter=20, progress=10 ** 9, autosave="None")
        sequences = [seq for seq, _ in dataset.test_set(epochs=1)] + [seq for seq, _ in dataset.validation_set(epochs=1)]
        many = predictor.top_k_batch(sequences, k=20)
        base = RNNBase.top_k_batch(predictor, sequences, k=20)
        assert [ids for ids, _ in many] == base and all(n == N_ITEMS for _, n in many)
        assert predictor.engine.query("cluster_rank_form") == 0 and predictor.top_k_batch([], k=5) == []
    finally:
        predictor.head.close(); predictor.engine.close()


def test_test_cli_reports_cluster_restricted_metrics(tmp_path):
    from sbr_amd import test as Te, train as T
    from sbr_amd.data import Evaluator
    root = make_dataset(str(tmp_path / "ds"), n_users=60, n_items=N_ITEMS)
    T.main(["-d", root] + BASE + ["--max_iter", "20", "--progress", "20", "--save", "All"])
    files = sorted(glob.glob(root + "models/*"))
    assert files
    predictor, dataset, args = trained_predictor(root, Te.test_command_parser)
    try:
        assert args.clusters == 4 and predictor.engine.query("cluster_rank_form") == 0
        for k in (10, 100):
            ev_cli = Te.run_tests(predictor, files[-1], dataset, args, k=k)
            assert predictor.engine.query("cluster_rank_form") == 1
            ev, ns, clusters = Evaluator(dataset, k=k), [], []
            for sequence, user_id in dataset.test_set(epochs=1):
                nv = int(len(sequence) / 2)
                (ids, n), = predictor.top_k_batch([sequence[:nv]], user_ids=[user_id], k=k)
                ev.add_instance([i[0] for i in sequence[nv:]], ids)
                ns.append(n)
                clusters.append(int(predictor.head.select(1)[0]))
            ev.nb_of_dp = np.mean(ns)
            for m in METRICS:
                assert ev.metrics[m]() == ev_cli.metrics[m](), (m, k)
            sizes = [len(c) for c in predictor.head.cluster_lists()]
            assert ev_cli.nb_of_dp == np.mean([sizes[c] for c in clusters]) and ev_cli.nb_of_dp < N_ITEMS
        # the command itself, at both depths: the same numbers for that checkpoint
        for k in (10, 100):
            res = Te.main(["-d", root] + BASE + ["-k", str(k), "--metrics", ",".join(METRICS)])
            got = dict(res)[files[-1]]
            ev_cli = Te.run_tests(predictor, files[-1], dataset, args, k=k)
            assert got == {m: ev_cli.metrics[m]() for m in METRICS}
    finally:
        predictor.head.close(); predictor.engine.close()
