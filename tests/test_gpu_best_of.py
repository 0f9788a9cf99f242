"""Whisper's best_of through ASRModel on the GPU, TINY with max_batch 8: a sampled attempt is one forked run on the fork handle and returns the
candidate fallback.pick_best selects among the plain (temperature, seed + j) decodes - same ids, same log-probability bits; the ladder forks its sampled rungs
only; submit() and transcribe_batch() agree with transcribe(); a model built without best_of refuses the keyword."""
import numpy as np
import pytest

from gpu_common import same_bits
from sonicscribe_amd import fallback, spec, synth
from sonicscribe_amd.asr import ASRModel

pytestmark = pytest.mark.gpu
N_NEW, T, SEED0 = 12, 0.8, 2 ** 64 - 2      # (the third fork's seed wraps to 0)


def wav(i, n):
    return synth.synth_pcm(i, n).astype(np.float32) / 32768.0


@pytest.fixture(scope="module")
def model():
    m = ASRModel.from_synthetic(spec.TINY, max_batch=8, max_ctx=1024, token_logprobs=True, sampling=True, best_of=3)
    yield m
    m.close()


@pytest.fixture(scope="module")
def plain(model):
    """the reference, once: the three plain decodes of (audio 0, T, SEED0 + j) through the dispatcher, one sample each"""
    from sonicscribe_amd import sampling
    a = wav(31, 80000)
    return [model.submit(a, max_new_tokens=N_NEW, detailed=True, temperature=T, seed=sampling.fork_seed(SEED0, j), best_of=1).result(timeout=120) for j in range(3)]


def test_the_winner_is_the_best_of_the_plain_decodes(model, plain):
    assert model.get_model_info()["best_of"] == 3 and len(model._fork_engines) == 1
    assert all((p.best_of, p.fork_index) == (1, 0) for p in plain)
    assert len({tuple(p.token_ids.tolist()) for p in plain}) >= 2, "the three seeds drew one transcript: the test shows nothing"
    avgs = [p.avg_logprob for p in plain]
    j = fallback.pick_best(avgs)
    a = wav(31, 80000)
    info = model.transcribe(a, max_new_tokens=N_NEW, temperature=T, seed=SEED0, best_of=3, return_debug_info=True)
    assert (info["best_of"], info["fork_index"], info["temperature"]) == (3, j, T)
    assert np.array_equal(info["token_ids"], plain[j].token_ids) and same_bits(info["token_logprobs"], plain[j].token_logprobs) and info["transcript"] == plain[j].text
    det = model.submit(a, max_new_tokens=N_NEW, detailed=True, temperature=T, seed=SEED0, best_of=3).result(timeout=120)      # submit() resolves to the same
    assert np.array_equal(det.token_ids, plain[j].token_ids) and same_bits(det.token_logprobs, plain[j].token_logprobs)
    assert (det.best_of, det.fork_index, det.attempts) == (3, j, 1) and det.fork_avg_logprobs.tolist() == avgs
    # the constructor's N is the default; two samples are the first two of three
    dflt = model.submit(a, max_new_tokens=N_NEW, detailed=True, temperature=T, seed=SEED0).result(timeout=120)
    assert dflt.best_of == 3 and np.array_equal(dflt.token_ids, det.token_ids)
    two = model.submit(a, max_new_tokens=N_NEW, detailed=True, temperature=T, seed=SEED0, best_of=2).result(timeout=120)
    assert two.best_of == 2 and two.fork_avg_logprobs.tolist() == avgs[:2] and np.array_equal(two.token_ids, plain[fallback.pick_best(avgs[:2])].token_ids)
    # temperature 0 never forks
    greedy = model.submit(a, max_new_tokens=N_NEW, detailed=True, temperature=0.0, best_of=3).result(timeout=120)
    assert (greedy.best_of, greedy.fork_index) == (1, 0)


def test_the_ladder_forks_its_sampled_rung(model, plain):
    a = wav(31, 80000)
    j = fallback.pick_best([p.avg_logprob for p in plain])
    keep = model.logprob_threshold
    model.logprob_threshold = 0.0                # no log-probability is above 0: every attempt fails, the last one is returned
    try:
        det = model.submit(a, max_new_tokens=N_NEW, detailed=True, temperature=(0.0, T), seed=SEED0, best_of=3).result(timeout=120)
    finally:
        model.logprob_threshold = keep
    assert (det.attempts, det.temperature, det.best_of, det.fork_index) == (2, T, 3, j)
    assert np.array_equal(det.token_ids, plain[j].token_ids) and same_bits(det.token_logprobs, plain[j].token_logprobs)


def test_transcribe_batch_packs_forked_runs(model):
    audios = [wav(40 + i, n) for i, n in enumerate((48000, 80000, 64000, 120000, 96000))]
    eng = model._fork_engines[0]
    runs = []
    real = eng.transcribe_batch
    eng.transcribe_batch = lambda *a, **kw: (runs.append(list(kw["forks"])), real(*a, **kw))[1]
    try:
        texts = model.transcribe_batch(audios, max_new_tokens=N_NEW, temperature=T, seed=5, best_of=3)
    finally:
        del eng.transcribe_batch
    assert runs == [[3, 3], [3, 3], [3]]         # floor(max_batch / best_of) = 2 audios per forked run
    single = [model.transcribe(a, max_new_tokens=N_NEW, temperature=T, seed=5, best_of=3) for a in audios]
    assert texts == single and len(set(texts)) >= 2


def test_a_model_without_best_of_refuses_the_keyword():
    m = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True, sampling=True)
    try:
        assert m.get_model_info()["best_of"] == 1 and m._fork_engines == []
        a = wav(31, 80000)
        for call in (lambda: m.transcribe(a, temperature=T, best_of=2), lambda: m.submit(a, temperature=T, best_of=1), lambda: m.transcribe_batch([a], temperature=T, best_of=2)):
            with pytest.raises(ValueError, match="best_of"):
                call()
        assert isinstance(m.transcribe(a, max_new_tokens=4, temperature=T, seed=1), str)
    finally:
        m.close()
    with pytest.raises(ValueError, match="best_of"):
        ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True, sampling=True, best_of=5)
    with pytest.raises(ValueError, match="best_of.*sampling"):
        ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True, best_of=2)
    with pytest.raises(ValueError, match="bulk"):
        ASRModel.from_synthetic(spec.TINY, max_batch=32, max_ctx=1024, token_logprobs=True, sampling=True, best_of=2, bulk=True)
