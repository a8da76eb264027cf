"""Dataset access + top-k metrics for the RNN path, Python 3.  Behaviour follows the reference's
helpers/data_handling.py:12-174 (on-disk format written by preprocess.py:153-214) and
helpers/evaluation.py:16-216; unlike the reference, sequence files are parsed ONCE into integer
arrays instead of re-splitting every text line every epoch (data_handling.py:142-145).
"""
import os
import random

import numpy as np

DEFAULT_DIR = "../../data/"      # data_handling.py:9


class SequenceGenerator(object):
    """Streams (sequence=[[item, rating], ...], user_id) from a `*_set_sequences` file whose lines
    are `user item rating item rating ...`; `epochs` is the fractional pass counter the training
    loop records (data_handling.py:139, rnn_base.py:312)."""

    def __init__(self, filename, shuffle=False):
        self.filename, self.shuffle, self.epochs = filename, shuffle, 0.0

    def load(self):
        self.users, self.items, self.ratings = [], [], []
        with open(self.filename, "r") as f:
            for line in f:
                tok = line.split()
                if not tok:
                    continue
                n = (len(tok) - 1) // 2
                self.users.append(tok[0])
                self.items.append(np.array(tok[1:1 + 2 * n:2], dtype=np.int64))
                self.ratings.append(np.array(tok[2:2 + 2 * n:2], dtype=np.float64))
        self.order = list(range(len(self.users)))

    def __call__(self, min_length=2, max_length=None, length_choice="max", subsequence="contiguous", epochs=np.inf):
        if not hasattr(self, "users"):
            self.load()
        counter = 0
        self.epochs = 0.0
        while counter < epochs:
            counter += 1
            print("Opening file ({})".format(counter))
            if self.shuffle:
                random.shuffle(self.order)
            for j, li in enumerate(self.order):
                self.epochs = counter - 1 + j / len(self.order)
                sequence = [[int(i), float(r)] for i, r in zip(self.items[li], self.ratings[li])]
                if len(sequence) < min_length:
                    continue
                this_max = len(sequence) if max_length is None else max_length
                if length_choice == "random":
                    length = np.random.randint(min_length, min(this_max, len(sequence)) + 1)
                elif length_choice == "max":
                    length = min(this_max, len(sequence))
                else:
                    raise ValueError('Unrecognised length_choice option. Authorised values are "random" and "max" ')
                if length < len(sequence):
                    if subsequence == "random":
                        sequence = [sequence[i] for i in sorted(random.sample(range(len(sequence)), length))]
                    elif subsequence == "contiguous":
                        start = np.random.randint(0, len(sequence) - length + 1)
                        sequence = sequence[start:start + length]
                    elif subsequence == "begining":
                        sequence = sequence[:length]
                    else:
                        raise ValueError('Unrecognised subsequence option. Authorised values are "random", '
                                         '"contiguous" and "begining".')
                yield sequence, self.users[li]


class NativeBatchBuilder(object):
    """Training batches built on the device (sbr_dataset_* / sbr_build_batch in include/sbr_rnn.h):
    the stand-in for `_gen_mini_batch(sequence_noise(dataset.training_set()))` + `_prepare_input`
    (rnn_base.py:373-420, rnn_one_hot.py:83-106, rnn_sampling.py:159-194, rnn_margin.py:112-147) for every option that leaves
    the batch plan of a pass computable on the host: --rf, --n_targets, --shuffle_targets, --db, --sampling_bias, and the
    sequence noise (--n_dropout, --n_swap, --n_shuf, --n_ratings: a device pass over the users before each pass is planned,
    sequence_noise.py:52-94), and --target_bias (the rows of a pass are then planned on the host by the library, the device
    packs them: sbr_dataset_set_target_bias).

    The training file is parsed once (SequenceGenerator.load) and uploaded as CSR.  Per pass the users are walked in
    file order, or reshuffled like data_handling.py:139-141 with --tshuffle; the walk prints the reference's
    "Opening file (n)" line and keeps `training_set.epochs` (the fractional pass counter the training loop records,
    rnn_base.py:312) up to date per batch.  `next()` makes the next batch the engine's current batch.

    sync: the parallel.DataParallel of a multi-rank run.  `batch_size` stays the GLOBAL one: every rank plans the same pass and
    its engine (local_batch, row_offset) builds its own rows of each batch -- plus all B targets and the S negatives of the
    sampled heads.  Everything the plan and the draws depend on is rank 0's, broadcast: the builder's seed (the noise passes'
    seeds derive from it), the --target_bias seed and the --tshuffle order of each pass.  Every rank draws from Python's generator
    as the single-process run does and rank 0's draws are the ones used."""

    def __init__(self, engine, training_set, n_items, batch_size, pop_db=None, sample_cdf=None, seed=None, ratings=False,
                 shuffle_targets=False, noise=None, keep_prob=None, n_targets=1, sync=None):
        from .engine import DeviceDataset
        if not hasattr(training_set, "users"):
            training_set.load()
        self.engine, self.ts, self.batch_size = engine, training_set, int(batch_size)
        lengths = np.array([len(x) for x in training_set.items], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        items = np.concatenate(training_set.items).astype(np.int32) if len(lengths) else np.zeros(0, np.int32)
        self.ds = DeviceDataset(engine, items, offsets, n_items)
        self.ds.set_tables(pop_db, sample_cdf)
        if ratings or shuffle_targets:      # --rf: the rating index rides beside the item index; --shuffle_targets
            r = (np.concatenate(training_set.ratings) if len(lengths) else np.zeros(0)) if ratings else None
            self.ds.set_options(r, shuffle_targets)
        self.sync = sync if (sync is not None and sync.world > 1) else None
        shared = (lambda v: v) if self.sync is None else self.sync.broadcast_seed
        self._target_bias, self.tb_seed = None, None
        if keep_prob is not None:           # --target_bias: rows planned on the host (a row may run out of targets)
            self.tb_seed = shared(int(seed if seed is not None else random.getrandbits(62)))
            self._target_bias = (np.array(keep_prob, dtype=np.float32), int(n_targets))
            self.ds.set_target_bias(keep_prob, n_targets, seed=self.tb_seed)
        self.n_users = len(lengths)
        self.noise = noise if (noise is not None and getattr(noise, "name", "") != "") else None      # a SequenceNoise
        self.seed = shared(int(seed if seed is not None else random.getrandbits(63)))
        self.passes, self.cursor, self.n_batches, self.built = 0, 0, 0, 0
        self._frac = np.zeros(0)
        self._before_pass = self.ds.get_state()      # the dataset's state in front of the pass in force (get_state)

    def _plan(self, again=False):
        """Plans the next pass; again=True (set_state): the pass in force once more -- same number, same order, no line printed."""
        if not again:
            self.passes += 1
            if self.sync is None or self.sync.rank == 0:
                print("Opening file ({})".format(self.passes))
            self._before_pass = self.ds.get_state()
        order = None
        if self.ts.shuffle:
            if not again:
                random.shuffle(self.ts.order)
            order = np.asarray(self.ts.order, dtype=np.int32)
            if self.sync is not None and not again:       # rank 0's order of this pass
                order = self.sync.broadcast_array(order, order.shape, "int32")
                self.ts.order = order.tolist()
        if self.noise is not None:      # this pass's noised copy of every sequence; the plan below sees its lengths
            nz = self.noise
            self.ds.noise_pass(nz.dropout, nz.swap, nz.shuf, nz.shuf_std, nz.ratings_perturb, seed=self.seed + 7919 * self.passes)
        self.n_batches = self.ds.plan_pass(order, self.batch_size)
        seg = self.ds.segments()
        # fraction of the pass consumed when batch b is complete: position of its last user in the walk
        pos = np.empty(self.n_users, dtype=np.int64)
        pos[np.arange(self.n_users) if order is None else order] = np.arange(self.n_users)
        self._frac = np.zeros(self.n_batches)
        if len(seg):
            last_user = np.zeros(self.n_batches, dtype=np.int64)
            last_user[seg[:, 3]] = seg[:, 0]               # later segments of a batch overwrite earlier ones
            self._frac = pos[last_user] / float(max(1, self.n_users))
        self.cursor = 0

    def __iter__(self):
        return self

    def __next__(self):
        guard = 0
        while self.cursor >= self.n_batches:
            self._plan()
            guard += 1
            if guard > 4 + self.batch_size:      # no pass can complete a batch: nothing to train on
                raise StopIteration
        b = self.cursor
        self.engine.build_batch(self.ds, b, self.seed + self.built)
        self.cursor += 1
        self.built += 1
        self.ts.epochs = self.passes - 1 + float(self._frac[b])
        return b

    next = __next__

    def get_state(self):
        """Everything the batches still to come depend on, as a dict of plain values: seed, passes, cursor, built, the user order and
        pass fraction of the training set, the --target_bias seed, and the dataset's state (DeviceDataset.get_state) as it was in
        front of the pass in force -- the pass itself is planned again by set_state."""
        return {"seed": int(self.seed), "passes": int(self.passes), "cursor": int(self.cursor), "built": int(self.built),
                "order": [int(u) for u in self.ts.order], "epochs": float(self.ts.epochs), "tb_seed": self.tb_seed,
                "batch_size": int(self.batch_size), "n_users": int(self.n_users), "dataset": self._before_pass}

    def set_state(self, d):
        """Stands where the builder that returned `d` stood: the next next() builds the batch it would have built.  The dataset's
        state goes back to what it was in front of the pass in force and that pass is planned again -- its noise pass seeds from
        seed + 7919 * passes and so repeats itself -- without its "Opening file" line.  ValueError, before anything changes, for
        a state of another training set, batch size or target selection."""
        if int(d["n_users"]) != self.n_users or int(d["batch_size"]) != self.batch_size or len(d["order"]) != len(self.ts.order):
            raise ValueError("builder state of %d users in batches of %d: this builder has %d users, batches of %d"
                             % (d["n_users"], d["batch_size"], self.n_users, self.batch_size))
        if (d["tb_seed"] is None) != (self._target_bias is None):
            raise ValueError("builder state %s --target_bias, this builder %s" % (("with" if d["tb_seed"] is not None else "without"),
                                                                                 ("with" if self._target_bias is not None else "without")))
        if sorted(d["order"]) != list(range(self.n_users)):
            raise ValueError("builder state: the user order is no permutation")
        if self._target_bias is not None:       # the seed the row planner draws from is the saved run's (this also empties the carried rows)
            self.tb_seed = int(d["tb_seed"])
            self.ds.set_target_bias(self._target_bias[0], self._target_bias[1], seed=self.tb_seed)
        self.ds.set_state(d["dataset"])
        self._before_pass = d["dataset"]
        self.seed, self.passes, self.built = int(d["seed"]), int(d["passes"]), int(d["built"])
        self.ts.order = [int(u) for u in d["order"]]
        self.cursor, self.n_batches, self._frac = 0, 0, np.zeros(0)
        if self.passes > 0:
            self._plan(again=True)
            if int(d["cursor"]) > self.n_batches:
                raise ValueError("builder state: cursor %d in a pass of %d batches" % (d["cursor"], self.n_batches))
            self.cursor = int(d["cursor"])
        self.ts.epochs = float(d["epochs"])

    def close(self):
        self.ds.close()


def sequences_csr(sequence_set):
    """(items int32 (nnz,), offsets int64 (n_users + 1,), ratings float64 (nnz,)) of a SequenceGenerator's file: the CSR form
    DeviceDataset takes, users in file order."""
    if not hasattr(sequence_set, "users"):
        sequence_set.load()
    lengths = np.array([len(x) for x in sequence_set.items], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = np.concatenate(sequence_set.items).astype(np.int32) if len(lengths) else np.zeros(0, np.int32)
    ratings = np.concatenate(sequence_set.ratings) if len(lengths) else np.zeros(0)
    return items, offsets, ratings


def make_device_dataset(engine, sequence_set, n_items, ratings=False):
    """A SequenceGenerator's sequences in HBM, as NativeBatchBuilder uploads the training set: items, offsets, and with --rf the
    ratings beside them (set_options).  What RNNEngine.evaluate reads for a validation or test set."""
    from .engine import DeviceDataset
    items, offsets, r = sequences_csr(sequence_set)
    ds = DeviceDataset(engine, items, offsets, n_items)
    if ratings:
        ds.set_options(r, False)
    ds.items = items       # host copy: the goals of the users come from it (ds.offsets is the dataset's own)
    return ds


class DataHandler(object):
    """Directory resolver + `stats` loader + item popularity cache (data_handling.py:12-102)."""

    def __init__(self, dirname, extended_training_set=False, shuffle_training=False):
        self.dirname = self._get_path(dirname)
        self.extended_training_set = extended_training_set
        train = "data/train_set_sequences+" if extended_training_set else "data/train_set_sequences"
        self.training_set = SequenceGenerator(self.dirname + train, shuffle=shuffle_training)
        self.validation_set = SequenceGenerator(self.dirname + "data/val_set_sequences")
        self.test_set = SequenceGenerator(self.dirname + "data/test_set_sequences")
        self._load_stats()

    def device_set(self, which, engine, ratings=False):
        """The DeviceDataset of the "validation" or "test" set for `engine` (data.make_device_dataset), made on first use and
        kept: one per set.  Another engine, or another --rf setting, replaces it."""
        cache = self.__dict__.setdefault("_device_sets", {})
        hit = cache.get(which)
        if hit is None or hit[0] is not engine or hit[1] != bool(ratings):
            if hit is not None:
                hit[2].close()
            source = {"validation": self.validation_set, "test": self.test_set, "training": self.training_set}[which]
            hit = cache[which] = (engine, bool(ratings), make_device_dataset(engine, source, self.n_items, ratings=ratings))
        return hit[2]

    @property
    def item_popularity(self):
        if not hasattr(self.training_set, "_item_pop"):
            cache = self.dirname + "data/training_set_item_popularity.npy"
            if os.path.isfile(cache):
                self.training_set._item_pop = np.load(cache)
            else:
                pop = np.zeros(self.n_items)
                with open(self.dirname + "data/train_set_triplets") as f:
                    for line in f:
                        pop[int(line.split()[1])] += 1
                self.training_set._item_pop = pop
                tmp = "%s.%d.tmp.npy" % (cache, os.getpid())      # (another rank may look for the cache while this one writes it)
                np.save(tmp, pop)
                os.replace(tmp, cache)
        return self.training_set._item_pop

    def _get_path(self, dirname):
        a, b = os.path.exists(dirname), os.path.exists(DEFAULT_DIR + dirname + "/")
        if a and b:
            print('WARNING: ambiguous directory name, both "' + dirname + '" and "' + DEFAULT_DIR + dirname +
                  '" exist. "' + dirname + '" is used.')
        if a:
            return dirname
        if b:
            return DEFAULT_DIR + dirname + "/"
        raise ValueError("Dataset not found")

    def _load_stats(self):
        with open(self.dirname + "data/stats", "r") as f:
            f.readline()                                    # column titles
            for obj in (self, self.training_set, self.validation_set, self.test_set):
                obj.n_users, obj.n_items, obj.n_interactions, obj.longest_sequence = map(int, f.readline().split()[1:])
        if self.extended_training_set:
            self.training_set.n_users, self.training_set.n_items = self.n_users, self.n_items
            self.training_set.n_interactions += (self.validation_set.n_interactions + self.test_set.n_interactions) // 2


class Evaluator(object):
    """Top-k metrics over (goal, predictions) instances (evaluation.py:16-216)."""

    def __init__(self, dataset, k=10):
        self.instances, self.dataset, self.k = [], dataset, k
        # evaluation.py:24-35: the names test.py's --metrics accepts
        self.metrics = {"sps": self.sps, "recall": self.average_recall, "precision": self.average_precision,
                        "ndcg": self.average_ndcg, "item_coverage": self.item_coverage, "user_coverage": self.user_coverage,
                        "blockbuster_share": self.blockbuster_share, "novelty": self.average_novelty, "assr": self.assr}

    def add_instance(self, goal, predictions):
        self.instances.append([list(goal), list(predictions)])

    def _top(self, prediction):
        return prediction[:min(len(prediction), self.k)]

    def average_precision(self):
        s = sum(len(set(g) & set(self._top(p))) / min(len(p), self.k) for g, p in self.instances if len(p) > 0)
        return s / len(self.instances)

    def average_recall(self):
        s = sum(len(set(g) & set(self._top(p))) / len(g) for g, p in self.instances if len(g) > 0)
        return s / len(self.instances)

    def average_ndcg(self):
        ndcg = 0.0
        for goal, prediction in self.instances:
            if len(prediction) > 0:
                dcg = max_dcg = 0.0
                for i, p in enumerate(self._top(prediction)):
                    if i < len(goal):
                        max_dcg += 1.0 / np.log2(2 + i)
                    if p in goal:
                        dcg += 1.0 / np.log2(2 + i)
                ndcg += dcg / max_dcg
        return ndcg / len(self.instances)

    def sps(self):
        return sum(int(g[0] in self._top(p)) for g, p in self.instances) / len(self.instances)

    def user_coverage(self):
        return sum(int(len(set(g) & set(self._top(p))) > 0) for g, p in self.instances) / len(self.instances)

    def get_correct_predictions(self):
        out = []
        for g, p in self.instances:
            out.extend(list(set(g) & set(self._top(p))))
        return out

    def item_coverage(self):
        return len(set(self.get_correct_predictions()))

    def average_novelty(self):
        """evaluation.py:90-101 ("Auralist"): -mean log2(popularity share) of the recommended items."""
        total = float(np.sum(self.dataset.item_popularity))
        nov = 0.0
        for _, p in self.instances:
            if len(p) > 0:
                top = np.asarray(self._top(p), dtype=np.int64)
                nov += float(np.sum(np.log2(self.dataset.item_popularity[top] / total))) / min(len(p), self.k)
        return -nov / len(self.instances)

    def get_rank_comparison(self):
        """evaluation.py:196-205: (position in the goal list, position in the recommendation list) pairs; needs full
        recommendation lists (test.py --save_rank)."""
        out = []
        for goal, prediction in self.instances:
            pos = np.argsort(prediction)[goal]
            out.extend(list(enumerate(pos)))
        return out

    def assr(self):
        """evaluation.py:207-216: average search-space reduction (1 without the clustering head)."""
        nb = getattr(self, "nb_of_dp", 0)
        return self.dataset.n_items / nb if nb and nb > 0 else 1

    def blockbuster_share(self):
        correct = self.get_correct_predictions()
        nb_pop = self.dataset.n_items // 100
        pop_items = set(np.argpartition(-self.dataset.item_popularity, nb_pop)[:nb_pop].tolist())
        if len(correct) == 0:
            return 0
        return len([i for i in correct if i in pop_items]) / len(correct)


class NativeEvaluator(Evaluator):
    """Evaluator over the per-user records RNNEngine.evaluate brings back from the device (include/sbr_rnn.h: sbr_evaluate)
    instead of (goal, predictions) lists: sps, recall, precision, user_coverage, item_coverage, blockbuster_share and ndcg come
    from the integer counts and the hit mask and equal, with ==, what Evaluator computes from the same ids -- the ratios are the
    same int / int divisions, added in user order by the same sequential sums.  `instances` is built on first use from the ids
    when they were fetched (want_ids); every other metric (novelty, get_rank_comparison, ...) is the base class's on them.
    add_instance still works: the instance's record is computed on the host and takes its place in the order."""

    def __init__(self, dataset, k=10):
        self._seg, self._inst, self._n = [], None, 0
        self._item_hits = None
        super(NativeEvaluator, self).__init__(dataset, k=k)      # (its metrics table binds the methods below)

    # ------------------------------------------------------------------ records in
    def add_records(self, rec, goal_len, goals=None, rows=None, item_hits=True):
        """rec: what RNNEngine.evaluate returned at this evaluator's k; goal_len (n,): len(goal) of every user; goals: their
        goal lists (only `instances` needs them); rows: the users of rec that take the next places (slice or index array; None =
        all of them, in order); item_hits=False: rec's per-item counts were already added with an earlier slice."""
        sel = slice(None) if rows is None else rows
        pick = lambda a: None if a is None else np.asarray(a)[sel]
        seg = {"n_pred": pick(rec["n_pred"]).astype(np.int64), "hits": pick(rec["hits"]).astype(np.int64),
               "first": pick(rec["first_hit"]).astype(np.int64), "glen": np.asarray(goal_len, dtype=np.int64).reshape(-1),
               "mask": pick(rec.get("hitmask")), "ids": pick(rec.get("ids")), "goals": goals}
        if len(seg["glen"]) != len(seg["n_pred"]):
            raise ValueError("goal_len must have one entry per user")
        if item_hits:
            ih = np.asarray(rec["item_hits"], dtype=np.int64)
            self._item_hits = ih.copy() if self._item_hits is None else self._item_hits + ih
        self._seg.append(seg)
        self._n += len(seg["n_pred"])
        self._inst = None

    def add_instance(self, goal, predictions):
        goal, top = list(goal), list(predictions)[:self.k]
        correct = set(goal) & set(top)
        bits = np.zeros((1, (self.k + 31) // 32), dtype=np.uint32)
        for i, p in enumerate(top):
            if p in goal:
                bits[0, i // 32] |= np.uint32(1 << (i % 32))
        if self._item_hits is None:
            self._item_hits = np.zeros(self.dataset.n_items, dtype=np.int64)
        for i in correct:
            self._item_hits[i] += 1
        self._seg.append({"n_pred": np.array([len(top)], np.int64), "hits": np.array([len(correct)], np.int64),
                          "first": np.array([int(len(goal) > 0 and goal[0] in top)], np.int64), "glen": np.array([len(goal)], np.int64),
                          "mask": bits, "ids": None, "goals": [goal], "host": [goal, list(predictions)]})
        self._n += 1
        self._inst = None

    # ------------------------------------------------------------------ instances, for everything the records do not carry
    @property
    def instances(self):
        if self._inst is None:
            out = []
            for seg in self._seg:
                if "host" in seg:
                    out.append(seg["host"])
                    continue
                if seg["ids"] is None or seg["goals"] is None:
                    raise RuntimeError("this metric needs the recommended ids: evaluate with want_ids=True and hand the goals over")
                out.extend([list(g), list(row[row >= 0])] for g, row in zip(seg["goals"], seg["ids"]))
            self._inst = out
        return self._inst

    @instances.setter
    def instances(self, value):      # (Evaluator.__init__ starts from an empty list)
        self._inst = None

    def _col(self, name):
        return np.concatenate([seg[name] for seg in self._seg]).tolist() if self._seg else []

    # ------------------------------------------------------------------ evaluation.py:37-88, 118-194 from the records
    def average_precision(self):
        return sum(h / p for h, p in zip(self._col("hits"), self._col("n_pred")) if p > 0) / self._n

    def average_recall(self):
        return sum(h / g for h, g in zip(self._col("hits"), self._col("glen")) if g > 0) / self._n

    def sps(self):
        return sum(self._col("first")) / self._n

    def user_coverage(self):
        return sum(int(h > 0) for h in self._col("hits")) / self._n

    def item_coverage(self):
        return 0 if self._item_hits is None else int(np.count_nonzero(self._item_hits))

    def blockbuster_share(self):
        nb_pop = self.dataset.n_items // 100
        pop_items = np.argpartition(-self.dataset.item_popularity, nb_pop)[:nb_pop]
        total = 0 if self._item_hits is None else int(self._item_hits.sum())
        if total == 0:
            return 0
        return int(self._item_hits[np.unique(pop_items)].sum()) / total

    def average_ndcg(self):
        # the discount of place i exactly as the base class computes it, one scalar call each; np.cumsum adds in order, and the
        # 0.0 of a place without a hit leaves the running sum as it is: dcg and max_dcg are the base class's sequential sums
        k = self.k
        disc = np.array([1.0 / np.log2(2 + i) for i in range(k)], dtype=np.float64)
        run = np.cumsum(disc)
        ndcg = 0.0
        for seg in self._seg:
            if seg["mask"] is None:
                raise RuntimeError("ndcg needs the hit mask: evaluate with want_mask=True")
            n = len(seg["n_pred"])
            bits = ((seg["mask"].astype(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1)[:, :k]
            dcg = np.cumsum(np.where(bits != 0, disc[None, :], 0.0), axis=1)[:, -1]
            m = np.minimum(seg["n_pred"], seg["glen"])
            for i in np.nonzero(seg["n_pred"] > 0)[0].tolist():
                ndcg += dcg[i] / (run[m[i] - 1] if m[i] > 0 else 0.0)
        return ndcg / self._n


class RankEvaluator(Evaluator):
    """Evaluator over the PLACE of every goal item in the complete ranking of its user (RNNEngine.evaluate_ranks, include/sbr_rnn.h:
    sbr_evaluate_ranks) instead of recommendation lists: one number per goal item answers every depth at once.  at(k) is the
    NativeEvaluator of depth k -- its records are derived from the ranks and equal what RNNEngine.evaluate returns at that k, so
    the seven record-based metrics equal, with ==, the ones of that call; the metrics table binds them at this evaluator's own k
    and adds "mrr".  get_rank_comparison() gives what the base class computes from full recommendation lists (test.py
    --save_rank), mrr() the mean reciprocal rank of the first goal item.  The ranks carry no ids: novelty and `instances`, which
    need the recommended ids, come from fetch_ids(k) -- a callable returning what RNNEngine.evaluate(k, want_ids=True) returns for
    the same users (RNNBase.native_rank_evaluator hands one over), called on first use; without one they raise RuntimeError."""

    RECORD_METRICS = ("sps", "recall", "precision", "ndcg", "item_coverage", "user_coverage", "blockbuster_share")

    def __init__(self, dataset, k=10, fetch_ids=None):
        super(RankEvaluator, self).__init__(dataset, k=k)
        self._rk, self._items, self._glen, self._nrk, self._at = [], [], [], [], {}
        self._fetch_ids, self._goals, self._ids_at = fetch_ids, [], {}
        table = {name: (lambda name=name: self.at(self.k).metrics[name]()) for name in self.RECORD_METRICS}
        table.update({"assr": self.assr, "novelty": self.average_novelty, "mrr": self.mrr})
        self.metrics = table

    # ------------------------------------------------------------------ ranks in
    def add_ranks(self, rec, goal_items):
        """rec: what RNNEngine.evaluate_ranks returned; goal_items: per user of rec, in order, the goal ids in sequence order
        (the DeviceDataset's host copy: items[off + L // 2 : off + L])."""
        off = np.asarray(rec["goal_off"], dtype=np.int64)
        glen = off[1:] - off[:-1]
        flat = np.concatenate([np.asarray(g, dtype=np.int64).reshape(-1) for g in goal_items]) if len(goal_items) else np.zeros(0, np.int64)
        if len(goal_items) != len(glen) or [len(g) for g in goal_items] != glen.tolist() or len(rec["ranks"]) != len(flat):
            raise ValueError("goal_items must hold the goal of every user of rec, as long as its ranks")
        self._rk.append(np.asarray(rec["ranks"], dtype=np.int64)); self._items.append(flat)
        self._glen.append(glen); self._nrk.append(np.asarray(rec["n_rankable"], dtype=np.int64))
        self._goals.extend(np.asarray(g).reshape(-1).tolist() for g in goal_items)
        self._at, self._ids_at = {}, {}

    def _flat(self):
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        glen = cat(self._glen)
        return cat(self._rk), cat(self._items), glen, cat(self._nrk), np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)

    def n_unrankable(self):
        """goal places whose item is never ranked (rank -1: excluded, NaN or -inf score)"""
        return int(sum(int(np.count_nonzero(r < 0)) for r in self._rk))

    # ------------------------------------------------------------------ any depth
    def at(self, k):
        """The NativeEvaluator of depth k: n_pred = min(k, n_rankable), hits = the distinct goal items with 0 <= rank < k,
        first_hit = goal[0] among them, hitmask bit `rank` per such item, item_hits their per-item counts."""
        k = int(k)
        if k not in self._at:
            rank, items, glen, nrk, off = self._flat()
            n = len(glen)
            user = np.repeat(np.arange(n, dtype=np.int64), glen)
            first_place = np.zeros(len(rank), dtype=bool)      # one place per distinct (user, item): a repeated item holds one rank
            first_place[np.unique(user * int(self.dataset.n_items) + items, return_index=True)[1]] = True
            sel = first_place & (rank >= 0) & (rank < k)
            mask = np.zeros((n, (k + 31) // 32), dtype=np.uint32)
            np.bitwise_or.at(mask, (user[sel], rank[sel] // 32), (np.uint32(1) << (rank[sel] % 32).astype(np.uint32)))
            head = rank[off[:-1]] if n else rank
            rec = {"n_pred": np.minimum(k, nrk).astype(np.int32), "hits": np.bincount(user[sel], minlength=n).astype(np.int32),
                   "first_hit": ((head >= 0) & (head < k)).astype(np.int32), "hitmask": mask, "ids": None,
                   "item_hits": np.bincount(items[sel], minlength=int(self.dataset.n_items)).astype(np.int32)}
            ev = NativeEvaluator(self.dataset, k=k)
            ev.add_records(rec, glen)
            self._at[k] = ev
        return self._at[k]

    def records(self, k):
        """the record dict at(k) is built from (what RNNEngine.evaluate returns at k, without ids)"""
        seg = self.at(k)._seg[0]
        return {"n_pred": seg["n_pred"].astype(np.int32), "hits": seg["hits"].astype(np.int32), "first_hit": seg["first"].astype(np.int32),
                "hitmask": seg["mask"], "item_hits": self.at(k)._item_hits.astype(np.int32)}

    # ------------------------------------------------------------------ the full ranking
    def get_rank_comparison(self):
        rank, _, glen, _, off = self._flat()
        return [(j, int(rank[off[u] + j])) for u in range(len(glen)) for j in range(int(glen[u]))]

    def mrr(self):
        rank, _, glen, _, off = self._flat()
        head = rank[off[:-1]].tolist()
        return sum(1.0 / (1 + r) if r >= 0 else 0.0 for r in head) / len(glen)

    def with_ids(self, k):
        """The NativeEvaluator of depth k over the ids themselves (fetch_ids(k)): what the ranks cannot serve -- novelty, instances."""
        k = int(k)
        if k not in self._ids_at:
            if self._fetch_ids is None:
                raise RuntimeError("this metric needs the recommended ids, which ranks do not carry: hand RankEvaluator a fetch_ids")
            ev = NativeEvaluator(self.dataset, k=k)
            ev.add_records(self._fetch_ids(k), self._flat()[2], goals=self._goals)
            self._ids_at[k] = ev
        return self._ids_at[k]

    def average_novelty(self):
        return self.with_ids(self.k).average_novelty()

    @property
    def instances(self):
        return self.with_ids(self.k).instances

    @instances.setter
    def instances(self, value):      # (Evaluator.__init__ starts from an empty list)
        pass

    # the base class's methods of the record-based metrics, at this evaluator's own k
    def sps(self): return self.at(self.k).sps()
    def average_recall(self): return self.at(self.k).average_recall()
    def average_precision(self): return self.at(self.k).average_precision()
    def average_ndcg(self): return self.at(self.k).average_ndcg()
    def user_coverage(self): return self.at(self.k).user_coverage()
    def item_coverage(self): return self.at(self.k).item_coverage()
    def blockbuster_share(self): return self.at(self.k).blockbuster_share()


class PositionEvaluator(object):
    """Metrics over the place of the NEXT item at every position of every sequence (RNNEngine.evaluate_positions, include/sbr_rnn.h:
    sbr_evaluate_positions): one (history, next item) pair per position where the other evaluators hold one instance per user.
    A position's history length is p, the number of items in front of the goal x_p.  An unrankable goal (rank -1) counts as a
    miss everywhere: no hit, reciprocal rank 0, gain 0.  Each position has ONE relevant item, so the ideal DCG is 1 and
    ndcg(k) is the mean of 1 / log2(2 + rank) over the positions with rank < k."""

    def __init__(self):
        self._rank, self._hist, self._nrk, self._users = [], [], [], 0

    def add_ranks(self, rec, lengths, min_history):
        """rec: what RNNEngine.evaluate_positions returned for min_history; lengths (n,): the length L of every user's sequence, in
        rec's order (a user has at most L - min_history positions: the result is checked against it)."""
        off = np.asarray(rec["pos_off"], dtype=np.int64)
        lengths, m = np.asarray(lengths, dtype=np.int64).reshape(-1), int(min_history)
        n_pos = off[1:] - off[:-1]
        if m < 1 or len(lengths) != len(n_pos) or len(rec["ranks"]) != off[-1] or len(rec["n_rankable"]) != off[-1] \
                or np.any(n_pos > np.maximum(0, lengths - m)):
            raise ValueError("lengths must hold the sequence length of every user of rec, and rec the positions min_history allows")
        self._rank.append(np.asarray(rec["ranks"], dtype=np.int64))
        self._nrk.append(np.asarray(rec["n_rankable"], dtype=np.int64))
        # position i of a user stands behind p = min_history + i items
        self._hist.append(m + np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], n_pos))
        self._users += len(n_pos)

    def add_events(self, rec, min_history=1):
        """rec: what SessionPool.replay_ranks returned ({"off", "ranks", "n_rankable", "events_before"}): one pair per replayed
        event, whose history length is the events its slot had in front of it (events_before -- not bounded by max_length: a
        session has no window).  Pairs with fewer than min_history events in front of them are dropped."""
        off = np.asarray(rec["off"], dtype=np.int64)
        rank, nrk = np.asarray(rec["ranks"], dtype=np.int64), np.asarray(rec["n_rankable"], dtype=np.int64)
        hist = np.asarray(rec["events_before"], dtype=np.int64)
        if len(off) < 1 or not (len(rank) == len(nrk) == len(hist) == off[-1]) or np.any(hist < 0):
            raise ValueError("rec must hold one rank, one n_rankable and one events_before per event of its off")
        keep = hist >= int(min_history)
        self._rank.append(rank[keep])
        self._nrk.append(nrk[keep])
        self._hist.append(hist[keep])
        self._users += len(off) - 1

    def _flat(self):
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        return cat(self._rank), cat(self._hist)

    def n_positions(self):
        return int(sum(len(r) for r in self._rank))

    def n_users(self):
        return self._users

    def n_unrankable(self):
        return int(sum(int(np.count_nonzero(r < 0)) for r in self._rank))

    @staticmethod
    def _rr(rank):
        return np.where(rank >= 0, 1.0 / (1.0 + np.maximum(rank, 0)), 0.0)

    def hit_rate(self, k):
        """the share of positions whose next item is among the first k of the ranking (sps at every position)"""
        rank, _ = self._flat()
        return int(np.count_nonzero((rank >= 0) & (rank < int(k)))) / len(rank)

    def mrr(self):
        rank, _ = self._flat()
        return float(self._rr(rank).sum()) / len(rank)

    def ndcg(self, k):
        rank, _ = self._flat()
        gain = np.where((rank >= 0) & (rank < int(k)), 1.0 / np.log2(2.0 + np.maximum(rank, 0)), 0.0)
        return float(gain.sum()) / len(rank)

    def by_history(self, k):
        """{"count", "hits", "rr"}: arrays over the history length h = 0 .. the longest one -- the positions with h items in front
        of the goal (int64), those of them with rank < k (int64), and the sum of their reciprocal ranks (float64)"""
        rank, hist = self._flat()
        size = int(hist.max()) + 1 if len(hist) else 0
        return {"count": np.bincount(hist, minlength=size).astype(np.int64),
                "hits": np.bincount(hist[(rank >= 0) & (rank < int(k))], minlength=size).astype(np.int64),
                "rr": np.bincount(hist, weights=self._rr(rank), minlength=size).astype(np.float64)}


class CandidateEvaluator(object):
    """Metrics over the place of every goal item among a candidate set of its user (RNNEngine.evaluate_candidates, include/sbr_rnn.h:
    sbr_evaluate_candidates) -- the sampled protocol: each positive against n_negatives items the user never interacted with.  A
    rank counts the candidates in front of the goal item, so one add_ranks answers every depth.  Per user the FIRST goal item is
    "the" positive of sps, ndcg and mrr (one relevant item: the ideal DCG is 1); recall looks at all of the user's distinct goal
    items.  An unrankable goal item (rank -1) is a miss everywhere.  The metrics table binds the depth-dependent ones at this
    evaluator's own k; at(k) gives all four at any depth."""

    def __init__(self, n_negatives=None, k=10):
        self.n_negatives, self.k = n_negatives, int(k)
        self._rk, self._items, self._glen, self._ncand = [], [], [], []
        self.metrics = {"sampled_sps": lambda: self.sps(self.k), "sampled_ndcg": lambda: self.ndcg(self.k),
                        "sampled_recall": lambda: self.recall(self.k), "sampled_mrr": self.mrr}

    def add_ranks(self, rec, goal_items):
        """rec: what RNNEngine.evaluate_candidates returned; goal_items: per user of rec, in order, the goal ids in sequence order
        (the DeviceDataset's host copy: items[off + L // 2 : off + L])."""
        off = np.asarray(rec["goal_off"], dtype=np.int64)
        glen = off[1:] - off[:-1]
        flat = np.concatenate([np.asarray(g, dtype=np.int64).reshape(-1) for g in goal_items]) if len(goal_items) else np.zeros(0, np.int64)
        if len(goal_items) != len(glen) or [len(g) for g in goal_items] != glen.tolist() or len(rec["ranks"]) != len(flat) \
                or len(rec["n_cand"]) != len(glen) or np.any(glen < 1):
            raise ValueError("goal_items must hold the goal of every user of rec, as long as its ranks")
        self._rk.append(np.asarray(rec["ranks"], dtype=np.int64)); self._items.append(flat)
        self._glen.append(glen); self._ncand.append(np.asarray(rec["n_cand"], dtype=np.int64))

    def _flat(self):
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        glen = cat(self._glen)
        return cat(self._rk), cat(self._items), glen, np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)

    def n_users(self):
        return int(sum(len(g) for g in self._glen))

    def n_unrankable(self):
        """goal places whose item is never ranked (rank -1: excluded, NaN or -inf score)"""
        return int(sum(int(np.count_nonzero(r < 0)) for r in self._rk))

    def n_short(self):
        """users with fewer than n_negatives rankable candidates: the draw ended at its attempt cap before n_negatives eligible
        items had come up (or a candidate scored NaN / -inf)"""
        if self.n_negatives is None:
            raise RuntimeError("n_short() needs the n_negatives this evaluator was made for")
        return int(sum(int(np.count_nonzero(c < int(self.n_negatives))) for c in self._ncand))

    def _head(self):
        rank, _, _, off = self._flat()
        return rank[off[:-1]]

    def sps(self, k):
        """the share of users whose first goal item has fewer than k candidates in front of it (HR@k of the sampled protocol)"""
        head = self._head()
        return int(np.count_nonzero((head >= 0) & (head < int(k)))) / len(head)

    def ndcg(self, k):
        head = self._head()
        gain = np.where((head >= 0) & (head < int(k)), 1.0 / np.log2(2.0 + np.maximum(head, 0)), 0.0)
        return float(gain.sum()) / len(head)

    def recall(self, k):
        """per user the share of its distinct goal items with a rank in [0, k), then the mean over the users"""
        rank, items, glen, _ = self._flat()
        n = len(glen)
        user = np.repeat(np.arange(n, dtype=np.int64), glen)
        first_place = np.zeros(len(rank), dtype=bool)      # one place per distinct (user, item): a repeated item holds one rank
        first_place[np.unique(user * (int(items.max()) + 1 if len(items) else 1) + items, return_index=True)[1]] = True
        distinct = np.bincount(user[first_place], minlength=n)
        hit = np.bincount(user[first_place & (rank >= 0) & (rank < int(k))], minlength=n)
        return float((hit / distinct).sum()) / n

    def mrr(self):
        head = self._head()
        return float(np.where(head >= 0, 1.0 / (1.0 + np.maximum(head, 0)), 0.0).sum()) / len(head)

    def at(self, k):
        """{"sampled_sps", "sampled_ndcg", "sampled_recall", "sampled_mrr"} at depth k"""
        return {"sampled_sps": self.sps(k), "sampled_ndcg": self.ndcg(k), "sampled_recall": self.recall(k), "sampled_mrr": self.mrr()}


class LikelihoodEvaluator(object):
    """The validation loss: reductions over the log-probability of held-out items (RNNEngine.evaluate_logprob and
    evaluate_positions_logprob, include/sbr_rnn.h: sbr_evaluate_logprob) -- the full-softmax negative log-likelihood (NLL) of the
    next item, the one number that compares models trained with different heads as probability models.  Every reduction runs in
    float64 on the host over the float32 values the device returned.  A goal that is not rankable (logp = -inf: excluded, NaN or
    -inf score, outside the catalogue) has no likelihood: it is counted in n_unrankable and left out of every mean."""

    def __init__(self):
        self._logp, self._first, self._hist, self._users = [], [], [], 0
        self.metrics = {"nll": self.nll, "ppl": self.perplexity, "first_nll": self.first_nll}

    def add_logprob(self, rec):
        """rec: what RNNEngine.evaluate_logprob returned: one logp per goal place, user j's at [goal_off[j], goal_off[j + 1])"""
        off = np.asarray(rec["goal_off"], dtype=np.int64)
        logp = np.asarray(rec["logp"], dtype=np.float64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or np.any(off[1:] < off[:-1]) or len(logp) != off[-1]:
            raise ValueError("rec must hold one logp per goal place of its goal_off")
        first = np.zeros(len(logp), dtype=bool)
        first[off[:-1][off[1:] > off[:-1]]] = True
        self._logp.append(logp); self._first.append(first); self._hist.append(np.full(len(logp), -1, dtype=np.int64))
        self._users += len(off) - 1

    def add_positions(self, rec, min_history):
        """rec: what RNNEngine.evaluate_positions_logprob returned for min_history: one logp per position, in order of p"""
        off = np.asarray(rec["pos_off"], dtype=np.int64)
        logp, m = np.asarray(rec["logp"], dtype=np.float64).reshape(-1), int(min_history)
        if m < 1 or len(off) < 1 or off[0] != 0 or np.any(off[1:] < off[:-1]) or len(logp) != off[-1]:
            raise ValueError("rec must hold one logp per position of its pos_off, and min_history >= 1")
        n_pos = off[1:] - off[:-1]
        first = np.zeros(len(logp), dtype=bool)
        first[off[:-1][n_pos > 0]] = True
        self._logp.append(logp); self._first.append(first)
        # position i of a user stands behind p = min_history + i items
        self._hist.append(m + np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], n_pos))
        self._users += len(n_pos)

    def _flat(self):
        cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
        return cat(self._logp, np.float64), cat(self._first, bool), cat(self._hist, np.int64)

    def n_users(self):
        return self._users

    def n_goals(self):
        return int(sum(len(x) for x in self._logp))

    @property
    def n_unrankable(self):
        """goal places without a likelihood (logp = -inf)"""
        return int(sum(int(np.count_nonzero(np.isneginf(x))) for x in self._logp))

    @staticmethod
    def _mean_nll(logp):
        keep = ~np.isneginf(logp)
        return float(-logp[keep].sum() / np.count_nonzero(keep)) if np.any(keep) else float("nan")

    def nll(self):
        """the mean of -logp over the rankable goals (nan when there is none)"""
        return self._mean_nll(self._flat()[0])

    def perplexity(self):
        """exp(nll())"""
        with np.errstate(over="ignore"):
            return float(np.exp(np.float64(self.nll())))

    def first_nll(self):
        """nll() over the FIRST goal item of every user only (the first position of a positions record): the analogue of sps"""
        logp, first, _ = self._flat()
        return self._mean_nll(logp[first])

    def by_history_length(self):
        """positions records only: {"count", "unrankable", "nll_sum"}, arrays over the history length h = 0 .. the longest one --
        the rankable positions with h items in front of the goal (int64), the unrankable ones (int64) and the sum of -logp over
        the rankable ones (float64): nll at h is nll_sum[h] / count[h]"""
        logp, _, hist = self._flat()
        if np.any(hist < 0):
            raise RuntimeError("by_history_length() needs position records (add_positions) only")
        size = int(hist.max()) + 1 if len(hist) else 0
        keep = ~np.isneginf(logp)
        return {"count": np.bincount(hist[keep], minlength=size).astype(np.int64),
                "unrankable": np.bincount(hist[~keep], minlength=size).astype(np.int64),
                "nll_sum": np.bincount(hist[keep], weights=-logp[keep], minlength=size).astype(np.float64)}
