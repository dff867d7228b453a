"""CPU tests of the receiver's host side: noise specification N1 restated in numpy (tests/noise_ref.py) against Philox4x32-10's
published known-answer vectors and the statistical bounds the specification implies; container format 3 (one policy job):
round trip, every refusal, and its separation from format 2."""
import struct

import numpy as np
import pytest

import noise_ref as NR


def test_philox4x32_10_known_answers():
    """The three known-answer vectors of Random123's kat_vectors for philox4x32, 10 rounds."""
    for ctr, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = tuple(int(w[0]) for w in NR.philox4x32_10(ctr, key))
        assert got == want, [hex(g) for g in got]


def test_counter_layout_of_the_specification():
    """counter = (j, step, start frame, stream id), key = (seed low, seed high): block j of ``words`` is one Philox call."""
    seed, sid, start, step = (7 << 32) | 1234, 5, 7, 3
    w = NR.words(seed, sid, start, step, 64)
    for j in (0, 9, 15):
        one = [int(v[0]) for v in NR.philox4x32_10((j, step, start, sid), (1234, 7))]
        assert w[4 * j:4 * j + 4].tolist() == one
    assert not np.array_equal(w, NR.words(seed, sid, start + 1, step, 64))
    assert not np.array_equal(w, NR.words(seed, sid + 1, start, step, 64))
    assert not np.array_equal(w, NR.words(seed, sid, start, step + 1, 64))
    assert not np.array_equal(w, NR.words(seed + (1 << 32), sid, start, step, 64))


def test_one_sample_step_is_standard_normal_within_the_bounds_of_the_specification():
    n = 15 * 128 * 128
    z = NR.normals(1234, 5, 7, 3, n)
    assert z.shape == (n,) and np.isfinite(z).all()
    mean, var, top = float(z.mean()), float(z.var()), float(np.abs(z).max())
    print(f"N1 seed 1234 stream 5 start 7 step 3: mean {mean:.5f} var-1 {var - 1:.5f} max|z| {top:.3f}")
    assert abs(mean) < 5 / np.sqrt(n)                      # 0.0101
    assert abs(var - 1) < 5 * np.sqrt(2 / n)               # 0.0143
    assert top <= np.sqrt(48 * np.log(2)) + 1e-12          # 5.77: u >= 2^-24


# ---- container format 3 ----------------------------------------------------------------------------------------

def key_frame(tag):
    """Strings of one key frame of one clip: [y_strings[5][2][1], z_strings[1]] with distinguishable contents."""
    ys = [[[bytes([tag, i, p]) * (1 + i + 2 * p)] for p in range(2)] for i in range(5)]
    return [ys, [bytes([tag]) * 3]]


SEGMENTS = [("key", 2), ("gen", 3), ("gen", 5), ("key", 2), ("gen", 5), ("gen", 5), ("gen", 5), ("key", 2), ("key", 1)]
N_KEY = 7


def packed(segments=SEGMENTS, n_key=N_KEY, **kw):
    import evc_amd  # noqa: F401
    from evc_amd import container
    args = dict(shape=(2, 2), codec=(0, 3), seed=(9 << 32) | 1234, stream_id=41, vid=17, q=4, thr=0.29, sampler="DDPM",
                subsample=100, denoise=True)
    args.update(kw)
    return container.pack_job(segments, [key_frame(k) for k in range(n_key)], **args)


def test_job_stream_round_trip():
    import evc_amd  # noqa: F401
    from evc_amd import container
    blob = packed()
    job = container.unpack_job(blob, expect_codec=(0, 3))
    assert job["segments"] == SEGMENTS and job["frames"] == 30 and job["shape"] == (2, 2)
    assert job["d"].tolist() == [1, 1] + [0] * 8 + [1, 1] + [0] * 15 + [1, 1, 1]
    assert (job["seed"], job["stream_id"], job["vid"], job["q"]) == ((9 << 32) | 1234, 41, 17, 4)
    assert job["thr"] == np.float32(0.29) and "%.2f" % job["thr"] == "0.29"
    assert (job["sampler"], job["subsample"], job["denoise"], job["noise_spec"]) == ("DDPM", 100, True, container.NOISE_N1)
    assert job["codec"] == (0, 3)
    assert job["key_strings"] == [key_frame(k) for k in range(N_KEY)]
    # the payload is exactly the strings: the sender's bit count
    assert container.payload_bits(job["key_strings"]) == 8 * sum(
        len(z) + sum(len(s[0]) for sl in ys for s in sl) for ys, (z,) in (key_frame(k) for k in range(N_KEY)))
    assert container.unpack_job(blob)["segments"] == SEGMENTS                    # no expectation: any codec tag
    other = container.unpack_job(packed(sampler="FPNDM", subsample=50, denoise=False, thr=31.5, q=0, vid=2 ** 32 - 1))
    assert (other["sampler"], other["subsample"], other["denoise"], other["thr"], other["q"], other["vid"]) == \
        ("FPNDM", 50, False, 31.5, 0, 2 ** 32 - 1)
    assert container.job_file_name(17, 4, job["thr"]) == "job_v17_q4_thr0.29.evc"


def test_job_stream_refusals():
    import evc_amd  # noqa: F401
    from evc_amd import container
    blob = packed()
    for cut in (3, 7, 8, 20, len(blob) - 1, len(blob) - 40):
        with pytest.raises(ValueError):
            container.unpack_job(blob[:cut])
    with pytest.raises(ValueError, match="trailing"):
        container.unpack_job(blob + b"\0")
    with pytest.raises(ValueError, match="not an EVC1"):
        container.unpack_job(b"EVC2" + blob[4:])
    for foreign in ((1, 3), (0, 2)):
        with pytest.raises(container.CodecMismatch):
            container.unpack_job(blob, expect_codec=foreign)
    with pytest.raises(ValueError, match="noise specification id 2"):
        container.unpack_job(packed(noise_spec=2))
    # inconsistent programs, both when writing and -- patched into the bytes -- when reading
    with pytest.raises(ValueError, match="two decoded frames"):
        packed([("key", 1), ("gen", 5)], 1)
    with pytest.raises(ValueError, match="key frames"):
        packed(SEGMENTS, N_KEY - 1)
    with pytest.raises(ValueError, match="1..5"):
        packed([("key", 2), ("gen", 6)], 2)
    head = 8 + struct.calcsize(container._JOB_HEAD)
    seg0 = head                                              # first segment: ("key", 2)
    bad = bytearray(blob); bad[seg0 + 1] = 1                 # noqa: E702  ("key", 1): the next "gen" has one frame before it
    with pytest.raises(ValueError, match="two decoded frames"):
        container.unpack_job(bytes(bad))
    bad = bytearray(blob); bad[seg0 + 3] = 4                 # noqa: E702  gen 3 -> gen 4: 31 frames against a header of 30
    with pytest.raises(ValueError, match="add up"):
        container.unpack_job(bytes(bad))
    bad = bytearray(blob); bad[seg0 + 2] = 0; bad[seg0 + 3] = 3    # noqa: E702  gen 3 -> key 3: 10 key frames, 7 strings
    with pytest.raises(ValueError, match="key frames"):
        container.unpack_job(bytes(bad))
    bad = bytearray(blob); bad[seg0] = 7                     # noqa: E702
    with pytest.raises(ValueError, match="segment kind"):
        container.unpack_job(bytes(bad))
    n_key_off = head - 4                                     # u16 n_key | u16 n_segments end the header
    bad = bytearray(blob); struct.pack_into("<H", bad, n_key_off, N_KEY + 1)     # noqa: E702
    with pytest.raises(ValueError, match="key frames"):
        container.unpack_job(bytes(bad))


def test_formats_2_and_3_do_not_mix():
    import evc_amd  # noqa: F401
    from evc_amd import container
    d = np.zeros(30, dtype=np.int64)
    d[:2] = 1
    keys = [[[[[b"ab", b"c"] for _ in range(2)] for _ in range(5)], [b"z0", b"z11"]] for _ in range(2)]
    blob2 = container.pack(d, keys, (2, 2), codec=(0, 3))
    d2, keys2, shape2 = container.unpack(blob2, expect_codec=(0, 3))               # format 2 reads as before
    assert (d2 == d).all() and keys2 == keys and shape2 == (2, 2)
    with pytest.raises(ValueError, match="not a job stream"):
        container.unpack_job(blob2)
    with pytest.raises(ValueError, match="format 3"):
        container.unpack(packed())
    with pytest.raises(ValueError, match="format 3"):
        container.read_codec(packed())


def test_noise_export_is_declared_bound_and_built():
    """The new C entry point: declared in the header, bound in lib.py, compiled from csrc/noise.hip, exported by the library."""
    import os
    import evc_amd  # noqa: F401
    from evc_amd import build, lib
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "evc_noise_normal_f32" in open(os.path.join(repo, "include", "evc_hip.h")).read()
    assert "evc_noise_normal_f32" in lib.HIP_SYMBOLS and "noise.hip" in build.HIP_SOURCES
    so = lib.hip_lib(require_device=False)
    assert so.evc_noise_normal_f32 is not None
    assert so.evc_noise_normal_f32(None, None, 1, 6, 0, 0, 0, None) == -1         # argument checks run before any launch
