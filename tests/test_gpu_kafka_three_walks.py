"""The three device walks of a Kafka produce request over the same inputs: the
classifier (kafka_classify_kernel), the compressed-set kernel
(kafka_inflate_kernel) and the deny-reply walk (deny_kafka_kernel), which
share one wire decoder and one message step (kernels/kafka_wire.h).

The sweep variable is the message set's size field, where a LimitReader count
and a sub-range end could disagree: for API versions 0, 1 and 2 and four fixed
message sets, the size runs from -2 to len(set) + 5 with the bytes unchanged,
so the set ends at every byte of every message and whatever follows (the next
partition, the next topic) is read from inside it.  That is 1,788 requests,
about 480 KB, in one batch; the host function answers 180 of them (all
distinct) and nothing to the other 1,608.

Every comparison is bit-exact.  Expected deny replies are the host function's
(_lib.kafka_deny_response, pinned by tests/test_kafka_response.py); expected
verdicts are the oracle's."""
import numpy as np
import pytest
import torch

from cilium_amd import _lib, api, gen
from cilium_amd._lib import ALLOW, DENY, PARSE_ERROR, PROTO_KAFKA

from test_gpu_deny_replies import K_CONN, _check, _Dev, _install_small, _produce_raw, _replies
from test_gpu_http import assert_same

pytestmark = pytest.mark.gpu

SETS = ("plain", "bad_crc", "snappy", "keyed")
ALIGNMENTS = (0, 5)  # the batch's first byte, mod 16: fields straddle chunk ends differently


def _sets(v):
    good = lambda n: gen.k_message(b"g" * n, version=v)  # noqa: E731
    return {
        "plain": good(20) + good(3) + good(33),
        "bad_crc": good(20) + gen.k_message(b"b" * 20, version=v, bad_crc=True) + good(20),
        "snappy": good(20) + gen.k_compressed(good(30) + good(40), 2, version=v) + good(20),
        "keyed": gen.k_message(b"v" * 10, key=b"key", version=v) + gen.k_message(b"", version=v),
    }


class _Sweep:
    def __init__(self):
        self.reqs, self.which = [], []
        for v in (0, 1, 2):
            one = gen.k_message(b"g" * 20, version=v)
            for name, ms in _sets(v).items():
                for size in range(-2, len(ms) + 6):
                    self.reqs.append(_produce_raw(v, len(self.reqs), [("t", [(1, size, ms), (2, len(one), one)]),
                                                                      ("u", [(3, -1, b"")])]))
                    self.which.append(name)
        self.which = np.array(self.which)
        self.replies = [_lib.kafka_deny_response(r) or b"" for r in self.reqs]
        self.cids = np.zeros(len(self.reqs), np.uint32)

    def placed(self, align):
        arena, offs, lens = gen.pack(self.reqs)
        return np.concatenate([np.zeros(align, np.uint8), arena]), offs + np.uint64(align), lens

    def workload(self, align):
        rules = [api.PortRuleKafka(api_key="produce", topic="t")]
        pol = api.policy_set(api.network_policy("ep", 1, ingress=[(9092, [api.port_rule(kafka=rules)])]))
        conns = gen.make_conns(1, 0, 9092, True, PROTO_KAFKA, [7], 9)
        return gen.Workload("t", *self.placed(align), self.cids, conns, pol)


@pytest.fixture(scope="module")
def sweep():
    return _Sweep()


@pytest.fixture(scope="module")
def oracle_verdicts(sweep, oracle):
    """(verdict, rule, consumed) of the oracle; they do not depend on where the batch lies."""
    return oracle.classify_workload(sweep.workload(0), 8)


def test_expected_replies_cover_both_outcomes(sweep):
    """The sweep cannot pass by everything answering nothing."""
    full = [e for e in sweep.replies if e]
    print("requests", len(sweep.reqs), "bytes", sum(map(len, sweep.reqs)), "non-empty", len(full),
          "distinct", len(set(full)), "empty", len(sweep.replies) - len(full))
    assert len(full) >= 150
    assert len(set(full)) >= 100


@pytest.mark.parametrize("align", ALIGNMENTS)
def test_deny_replies_equal_host(engine, sweep, align):
    _install_small(engine)
    arena, offs, lens = sweep.placed(align)
    D = _Dev(arena, offs, lens, np.full(len(sweep.reqs), K_CONN, np.uint32))
    assert (D.arena.data_ptr() + int(offs[0])) % 16 == align
    d_v = torch.full((D.n,), DENY, dtype=torch.uint8, device=D.arena.device)
    out = _replies(engine, D, d_v)
    _check(sweep.replies, out, int(out[3][0]))


@pytest.mark.parametrize("align", ALIGNMENTS)
def test_classification_equals_oracle(engine, sweep, oracle_verdicts, align):
    w = sweep.workload(align)
    engine.update_policy(w.policy)
    engine.set_connections(w.conns)
    got = engine.classify(w.arena, w.offsets, w.lengths, w.conn_ids)
    assert_same(got, oracle_verdicts, w)


def test_oracle_takes_both_paths_through_the_compressed_set(sweep, oracle_verdicts):
    """The compressed set's requests are both failed (the inflate kernel's
    error path) and decided (its decode path) somewhere in the sweep."""
    v = oracle_verdicts[0][sweep.which == "snappy"]
    assert (v == PARSE_ERROR).any()
    assert ((v == ALLOW) | (v == DENY)).any()
