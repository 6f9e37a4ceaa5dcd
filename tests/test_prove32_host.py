"""CPU tier of the slab32 prover: the keyed samplers' word-to-coefficient maps (rzk_chacha.h,
rzk_gauss.h, rzk_dgauss.h) evaluated at the extremes of every argument the 32-bit entry points accept and on a seeded
sweep, compiled with g++ under -fsanitize=address,undefined into tests/prove32/prove32_driver.cpp and run as a process.
What it establishes: every value lies inside int32, so rzk_sample_*_keyed32_dev needs no range rule of its own."""
import math
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SWEEP = 200000
Q_MIN, Q_DEFAULT, Q_MAX = 3, 3515337053, 4294606851


@pytest.fixture(scope="module")
def maxima(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the prove32 driver")
    exe = str(tmp_path_factory.mktemp("prove32") / "prove32_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "prove32", "prove32_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, "20261020", str(SWEEP)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    out = {}
    for line in res.stdout.splitlines():
        name, mx, n, misfit = line.split()
        out[name] = (int(mx), int(n), int(misfit))
    print(res.stdout)   # the maxima DESIGN.md section 20 quotes
    return out


def test_every_map_is_reported(maxima):
    assert sorted(maxima) == sorted(["uniform_qmin", "uniform_qdefault", "uniform_qmax", "gauss_f64_sigma_2p26",
                                     "gauss_f32_sigma_below_2p19", "dgauss_tail_bound_sigma_2p26", "dgauss_trial_sigma_2p26"])
    for name, (_, n, _) in maxima.items():
        assert n >= 2, name


def test_every_value_fits_int32(maxima):
    for name, (mx, n, misfit) in maxima.items():
        assert mx < 2 ** 31, (name, mx)
        assert misfit == 0, (name, misfit, n)


@pytest.mark.parametrize("name,q", [("uniform_qmin", Q_MIN), ("uniform_qdefault", Q_DEFAULT), ("uniform_qmax", Q_MAX)])
def test_uniform_reaches_exactly_half(maxima, name, q):
    """bound = h is the largest the entry points take: the all-zero words give -h, and nothing exceeds h."""
    assert maxima[name][0] == (q - 1) // 2 < 2 ** 31


def test_gauss_f64_maximum_is_the_53_bit_radius(maxima):
    """u0 >= 2^-53, so R <= 2^26 sqrt(2 * 53 ln 2) = 5.75e8; the sweep of angles reaches it at angle 0 (or half a turn)."""
    r = 2.0 ** 26 * math.sqrt(2 * 53 * math.log(2))
    mx = maxima["gauss_f64_sigma_2p26"][0]
    assert mx <= r + 1 and mx >= r - 2, (mx, r)
    assert r < 5.8e8


def test_gauss_f32_maximum_is_the_64_bit_radius(maxima):
    """u0 >= 2^-64, sigma < 2^19: R <= 2^19 sqrt(2 * 64 ln 2) = 4.94e6, with the relative error of the float form."""
    r = 2.0 ** 19 * math.sqrt(2 * 64 * math.log(2))
    mx = maxima["gauss_f32_sigma_below_2p19"][0]
    assert r * (1 - 1e-5) <= mx <= r * (1 + 1e-5), (mx, r)


def test_dgauss_tail_bound(maxima):
    """Every candidate is k x + y <= 8 k - 1 with k the least integer >= sigma sqrt(2 ln 2): 9.42 sigma at sigma = 2^26."""
    k = math.ceil(2 ** 26 * math.sqrt(2 * math.log(2)))
    bound = maxima["dgauss_tail_bound_sigma_2p26"][0]
    assert abs(bound - (8 * k - 1)) <= 8, (bound, k)          # (k by integer arithmetic in the header; the float here is a check)
    assert bound < 2 ** 30
    assert maxima["dgauss_trial_sigma_2p26"][0] <= bound
    assert maxima["dgauss_trial_sigma_2p26"][0] == bound      # the all-one words give x = 7 and the largest y
