"""The H.265 kernels (k_h265_mc, k_h265_ctu_rows, k_h265_ctu_grid, k_h265_deblock, k_h265_sao) against the CPU
oracle at the record level (tests/_h265_records.py): the records of real parses, their value fields mutated far
past what tools/h265gen writes, submitted by hand to both back ends; the frames must be equal byte for byte, the
whole width x height frame of every picture.  The cases, seeds and the domain cap are those of
tests/test_h265_records_cpu.py."""
import pytest

import _h265_records as R
from test_h265_cpu import SMALL


def _check(family, stream, seed, device=0):
    rec, want, viol = R.case(family, stream, seed)
    if viol:
        return 0  # outside the reference's defined domain (at most one case in ten: test_domain_cap)
    got = R.hip_replay(rec, device)
    diff = R.first_difference(rec, want, got)
    assert diff is None, f"{family} on {stream}, seed {seed} (oracle vs gfx950):\n{diff}"
    return 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_hip_replay_matches_oracle(built, name):
    """Unmutated: the hand-submitted, unstaged path, from the same seeded frames on both sides."""
    assert _check(None, name, 0) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("stream", R.STREAMS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_hip_mutated_records_match_oracle(built, family, stream):
    compared = sum(_check(family, stream, seed) for seed in R.seeds(family))
    print(f"{family} on {stream}: {compared} of {len(R.seeds(family))} seeds compared")


@pytest.mark.gpu
@pytest.mark.parametrize("stream", R.VARIANT_STREAMS)
@pytest.mark.parametrize("env", [{"M2DEC_AMD_H265_WAVES": "2"}, {"M2DEC_AMD_H265_CTU_GRID": "0"},
                                 {"M2DEC_AMD_H265_WAVES": "2", "M2DEC_AMD_H265_CTU_GRID": "0"}],
                         ids=["one_wave_per_plane", "rows", "one_wave_rows"])
def test_hip_all_families_under_switches(built, monkeypatch, env, stream):
    """Every family at once with one wave per plane in the CTU kernels, with P / B pictures through the row kernel,
    and both (the back end reads its environment when it is created)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for seed in R.SEEDS:
        _check("all", stream, seed)
