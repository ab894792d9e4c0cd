"""The generator's default draws are frozen: edge264_amd/synth.py's opt-in options (the range ends) may not move a single byte of the
packets that bench.py and the seeded tests get when those options are unset.  The digests below were taken before the options existed."""
import hashlib

import pytest

from edge264_amd import packet as P, synth

ALL_I = (P.MB_I8x8, P.MB_I4x4, P.MB_I16x16)
BENCH_I = (P.MB_I4x4, P.MB_I8x8, P.MB_I16x16)
BENCH = dict(t8x8=True, i_kinds=BENCH_I, num_refs=2, residual_prob=0.3)  # bench.py's skw
BENCH_C1 = dict(i_kinds=(P.MB_I4x4,), residual_prob=1.0, deblock=False)
BENCH_C3 = dict(t8x8=True, scaling=True, weighted=1, num_refs=2, residual_prob=0.3, i_kinds=ALL_I)

# (name, width, height, seed, picture types, options)
CONFIGS = [
    ("bench_1080p", 120, 68, 1234, "IP", BENCH),
    *[(f"bench_variant{v}", 12, 8, 1234 + v, "IPPPPPPP", BENCH) for v in range(4)],
    ("bench_configs1", 12, 8, 4321, "IIII", BENCH_C1),
    ("bench_configs3", 12, 8, 4321, "IPBBPBBP", BENCH_C3),
    # test_hip_parity.CASES
    ("intra4x4_16x16", 6, 5, 0, "III", dict()),
    ("intra8x8", 6, 5, 0, "III", dict(i_kinds=ALL_I, t8x8=True)),
    ("pcm", 6, 5, 0, "II", dict(pcm_prob=0.2)),
    ("scaling_lists", 6, 5, 0, "II", dict(scaling=True, i_kinds=ALL_I)),
    ("ippp", 6, 5, 0, "IPPPP", dict()),
    ("ippp_t8x8_scaling", 6, 5, 0, "IPPPP", dict(t8x8=True, scaling=True)),
    ("ippp_explicit_wp", 6, 5, 0, "IPPPP", dict(weighted=1)),
    ("ibbp", 6, 5, 0, "IPBBPBB", dict()),
    ("ibbp_explicit_wp", 6, 5, 0, "IPBBPBB", dict(weighted=1, t8x8=True)),
    ("ibbp_implicit_wp", 6, 5, 0, "IPBBPBB", dict(weighted=2, t8x8=True, scaling=True)),
    ("slices_idc2", 6, 5, 0, "IPBBP", dict(slices_per_frame=4, deblock_idc=2)),
    ("slices_idc0", 6, 5, 0, "IPBBP", dict(slices_per_frame=4, deblock_idc=0)),
    ("slices_scaling_explicit", 6, 5, 0, "IPBBP", dict(slices_per_frame=6, weighted=1, scaling=True, t8x8=True, i_kinds=ALL_I)),
    ("slices_scaling_implicit", 6, 5, 0, "IPBBP", dict(slices_per_frame=6, weighted=2, scaling=True, t8x8=True, i_kinds=ALL_I)),
    ("filter_offsets", 6, 5, 0, "IPB", dict(filter_offsets=(6, -4))),
    ("no_deblock", 6, 5, 0, "IPB", dict(deblock=False)),
    # the stress ones
    ("stress_explicit", 6, 5, 1, "IPBBP", dict(stress=True, weighted=1, t8x8=True, scaling=True, i_kinds=ALL_I)),
    ("stress_implicit_far_mv", 6, 5, 1, "IPBBP", dict(stress=True, weighted=2, t8x8=True, mv_range=400)),
    ("stress_pcm_slices", 7, 4, 2, "IPBBP", dict(stress=True, pcm_prob=0.2, slices_per_frame=3, qp_base=51, filter_offsets=(-12, 12),
                                                 weighted=1, scaling=True, num_refs=3)),
]

DIGESTS = {
    "bench_1080p": "ec7e1fecfca106ef70e7d3c4",
    "bench_variant0": "6e39bee6a0c5170c35db3874",
    "bench_variant1": "948f3ae50f684023abfdd522",
    "bench_variant2": "153864034244d87bd0ea83b4",
    "bench_variant3": "5c0c4e7f05f0ee26018f14ee",
    "bench_configs1": "235c476f37db088542e3fbf1",
    "bench_configs3": "fb7e1cbea3e56ad0bf5c36e8",
    "intra4x4_16x16": "873480eb0708a07d402f1d05",
    "intra8x8": "803c7c1aeceb58cdb80db92d",
    "pcm": "5add62147e5fcf50bc1e2974",
    "scaling_lists": "335b84f9302aec4723c8bb30",
    "ippp": "6a640804614770f72b7ea71c",
    "ippp_t8x8_scaling": "e48378f07a9edae91afe897f",
    "ippp_explicit_wp": "1004c43b309bc3cd04c2f5e3",
    "ibbp": "53880850713bb7fed204c204",
    "ibbp_explicit_wp": "14477c017a50a4fd37a91694",
    "ibbp_implicit_wp": "591764751f9d0a54bf1b71f2",
    "slices_idc2": "f49bae81842537d26b225dec",
    "slices_idc0": "5a72e208d90d11d1647c27d1",
    "slices_scaling_explicit": "fde6e5e36270f7654f6b18de",
    "slices_scaling_implicit": "857a3d481a250492c3426e66",
    "filter_offsets": "600cf9284e8a3b7eab090155",
    "no_deblock": "53c175857111c9620b5f9c29",
    "stress_explicit": "c5dc92f81b65f92701021393",
    "stress_implicit_far_mv": "f111a26b24056bcda3687f25",
    "stress_pcm_slices": "362666e497a86d5a9e7794f3",
}


def digest(w, h, seed, pattern, kw):
    s = synth.StreamSynth(w, h, seed, **kw)
    m = hashlib.sha256()
    for t in pattern:
        m.update(s.next_frame(t))
    return m.hexdigest()[:24]


@pytest.mark.parametrize("name,w,h,seed,pattern,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_default_draws_unchanged(name, w, h, seed, pattern, kw):
    assert digest(w, h, seed, pattern, kw) == DIGESTS[name]
