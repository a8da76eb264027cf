"""The yardstick of tests/test_gpu_trained_shape.py, checked without a GPU: for every case of that file, from the float64 oracle and
the float32 torch restatement alone (tests/trained_shape.py),

  - the float32 reference itself survives the parameters (finite cost and gradients): the trained-shaped edit moves biases, W_out and
    the output bias only -- larger recurrent weights make the recurrence chaotic and leave no float32 yardstick at all;
  - its own error is at most a tenth of the bar the engine is held to, so a pass there cannot be the reference's noise;
  - the model IS in the regime the cases are for: logits of a row over 20 nats and more, a peaked softmax, saturated states
    (GRU / Vanilla) or saturated gates (LSTM);
  - the ranking check at gap = 1e-3 compares three rows in four at least."""
import numpy as np
import pytest

import trained_shape as TS


@pytest.mark.parametrize("name", TS.IDS)
def test_reference_and_regime(name):
    c = TS.CASES[TS.IDS.index(name)]
    r = TS.reference(name, True)
    s, kw = r["stats"], c["kw"]
    print("trained shape", name, "floor_default", r["floor_default"], "floor_trained", r["floor_trained"], "ratio", r["ratio"], s)
    assert r["finite"]
    for q, bar in r["bar"].items():
        assert np.isfinite(r["floor_trained"][q]) and r["floor_trained"][q] <= 0.1 * bar, (q, r["floor_trained"][q], bar)
    assert s["logit_range_row_median"] >= 20.0, s       # (the median over the rows of each row's span: no less than the batch's span)
    assert s["logit_range"] >= s["logit_range_row_median"]
    if kw["loss"] == "CCE":
        assert s["top_prob_median"] >= 0.5, s
    if kw["cell"] == "LSTM":
        assert s["gates_saturated"] >= 0.05, s
    else:
        assert s["h_saturated"] >= 0.15, s
    assert s["rows_compared"] >= 0.75 * kw["B"], s


def test_the_trained_edit_touches_biases_and_the_output_layer_only():
    import parity_util as PU
    from oracle import rnn_oracle as O
    for cell, layers, kw in (("LSTM", [20, 12], {}), ("GRU", [20], dict(emb=6)), ("Vanilla", [20], dict(bi=True))):
        a, _, ba = PU.build_case(cell, layers, "CCE", 61, 9, 5, **kw)
        b, _, bb = PU.build_case(cell, layers, "CCE", 61, 9, 5, trained=TS.TRAINED, **kw)
        assert all(np.array_equal(ba[k], bb[k]) for k in ba)          # the batch is the same draw
        names = [n for n, _ in O.model_param_shapes(cell, layers, 61, 61, kw.get("emb", 0), 1, kw.get("bi", False))]
        assert len(names) == len(a) == len(b)
        for n, p, q in zip(names, a, b):
            moved = n in ("out.W", "out.b") or (n[0] == "l" and n.split(".")[1].startswith("b_"))
            assert np.array_equal(p, q) != moved, n
            assert np.array_equal(q, q.astype(np.float32).astype(np.float64)), n      # still float32 values
        W, Wt, bo = a[-2], b[-2], b[-1] - a[-1]
        assert np.abs(Wt - 8.0 * W).max() <= 1e-6 * np.abs(Wt).max()
        assert 11.5 <= bo.max() - bo.min() <= 12.5                     # the Zipf profile: span nats between the first and the last item


@pytest.mark.parametrize("name,cell,layers", TS.SESSION_MODELS, ids=[m[0] for m in TS.SESSION_MODELS])
def test_session_reference(name, cell, layers):
    r = TS.session_reference(cell, tuple(layers))
    print("trained shape sessions", name, r)
    for q, bar in r["bar"].items():
        assert np.isfinite(r["floor_trained"][q]) and r["floor_trained"][q] <= 0.1 * bar, (q, r)
