"""Host tests of ``keystrings.py``: the one place that walks ``[y_strings[5][2][B], z_strings[B]]``."""
import numpy as np
import pytest


def strings_of(rng, n_clips):
    """5 x 2 y strings and a z string per clip, 0..6 random bytes each, two of them emptied on purpose."""
    mk = lambda: bytes(rng.integers(0, 256, int(rng.integers(0, 7)), dtype=np.uint8))      # noqa: E731
    ys = [[[mk() for _ in range(n_clips)] for _ in range(2)] for _ in range(5)]
    ys[0][1][0] = ys[4][0][n_clips - 1] = b""
    return [ys, [mk() for _ in range(n_clips)]]


@pytest.mark.parametrize("n_clips", [1, 2, 3])
def test_split_and_merge_round_trip_and_the_three_bit_counts_agree(n_clips):
    from evc_amd import container, elic, keystrings as KS
    batch = strings_of(np.random.default_rng(n_clips), n_clips)
    frames = KS.split(batch)
    assert len(frames) == n_clips
    for b, f in enumerate(frames):                       # frame b alone: the same nesting with one clip
        assert f == [[[[batch[0][sl][p][b]] for p in range(2)] for sl in range(5)], [batch[1][b]]]
    assert KS.merge(frames) == batch and KS.split(KS.merge(frames)) == frames
    assert KS.merge([batch]) == batch
    # the given order is the order of the clip axis, and batches merge like frames
    back = KS.merge(frames[::-1])
    assert KS.split(back) == frames[::-1] and (back == batch) == (n_clips == 1)
    assert KS.merge([KS.merge(frames[:1]), KS.merge(frames[1:])] if n_clips > 1 else frames) == batch
    want = 8 * (sum(len(s) for sl in batch[0] for p in sl for s in p) + sum(len(z) for z in batch[1]))
    assert KS.bits(batch) == elic.count_bits(batch) == container.payload_bits([batch]) == want
    assert KS.bits(frames) == container.payload_bits(frames) == sum(elic.count_bits(f) for f in frames) == want
    assert KS.bits([]) == container.payload_bits([]) == 0


def test_flat_tells_frames_apart_by_any_single_string_and_the_caller_by_q():
    from evc_amd import keystrings as KS
    a = strings_of(np.random.default_rng(5), 1)
    assert KS.flat(a) == KS.flat(KS.split(a)[0]) and len(KS.flat(a)) == 11 and all(isinstance(s, bytes) for s in KS.flat(a))
    for sl in range(5):
        for p in range(2):
            b = KS.split(a)[0]
            b[0][sl][p][0] += b"\x01"
            assert KS.flat(b) != KS.flat(a), (sl, p)
    b = KS.split(a)[0]
    b[1][0] += b"\x01"
    assert KS.flat(b) != KS.flat(a)
    # moving a byte from one string to its neighbour keeps the bytes and changes the frame
    b = KS.split(a)[0]
    b[0][1][0][0], b[0][1][1][0] = b"xy", b"z"
    c = KS.split(a)[0]
    c[0][1][0][0], c[0][1][1][0] = b"x", b"yz"
    assert KS.flat(b) != KS.flat(c) and KS.bits(b) == KS.bits(c)
    # the receiver names a key frame (q, strings): equal strings under another q are another frame
    assert (3,) + KS.flat(a) != (4,) + KS.flat(a)


def test_the_receiver_names_key_frames_by_q_and_bytes():
    """``decode_jobs(share=True)``'s identity: equal (q, strings) -> one name, whichever job asks; another q -> another name."""
    from evc_amd import keystrings as KS
    from evc_amd.decoder import _JobRounds
    run = _JobRounds.__new__(_JobRounds)
    run.key_names = {}
    a, b = strings_of(np.random.default_rng(5), 1), strings_of(np.random.default_rng(6), 1)
    assert run.key_name(3, a) == run.key_name(3, KS.merge([a])) == ("key", 3, 0)
    assert run.key_name(4, a) == ("key", 4, 1) and run.key_name(3, b) == ("key", 3, 2) and run.key_name(3, a) == ("key", 3, 0)


def test_write_and_read_are_one_order_and_the_reader_refuses_to_run_past_the_end():
    from evc_amd import keystrings as KS
    batch = strings_of(np.random.default_rng(9), 3)
    out = []
    for b in range(3):
        KS.write(out, batch, b)
    blob = b"head" + b"".join(out)
    z0 = batch[1][0]
    assert blob[4:8 + len(z0)] == len(z0).to_bytes(4, "little") + z0                 # clip 0 starts with its z string
    reader = KS.Reader(blob, 4, "thing")
    assert KS.read(reader, 3) == batch
    reader.end()
    assert [KS.read(r) for r in [KS.Reader(blob, 4, "thing")] * 3] == KS.split(batch)   # clip after clip: one frame each
    for cut in range(4, len(blob)):
        with pytest.raises(ValueError, match="^truncated thing$"):
            KS.read(KS.Reader(blob[:cut], 4, "thing"), 3)
    with pytest.raises(ValueError, match="^trailing bytes in thing$"):
        KS.Reader(blob + b"\0", len(blob), "thing").end()
    r = KS.Reader(b"\x01\x02\x03", 0, "thing")
    assert r.unpack("<BH") == (1, 0x0302) and r.off == 3
    with pytest.raises(ValueError, match="^truncated thing$"):
        r.unpack("<B")
