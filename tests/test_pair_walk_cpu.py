"""The pair walk of a paired run (kbbq_amd/csrc/cli_pair_walk.h): which reads of which batches are mates, as the runs that
--pair-overlap and --pair-correct hand to the engine.  Exercised without a GPU through the binary's hidden --io-test pair-runs
helper, against a walk by brute force: every pair gets its (batch, index) on either side, and maximal runs are grouped."""
import os
import random
import subprocess

import pytest

import common

CLI = os.environ.get("KBBQ_CLI", os.path.join(common.ROOT, "kbbq_amd", "kbbq"))

INTERLEAVED = [[6], [3, 3], [1, 1], [2, 1, 1, 2], [1, 2, 1], [5, 1, 4]]
TWO_FILES = [([4, 3], [4, 3]), ([4, 4], [3, 5]), ([1] * 6, [6]), ([8], [2, 2, 2, 2])]


def random_cases():
    rng = random.Random(20251021)

    def partition(total):
        sizes = []
        while total:
            sizes.append(rng.randint(1, min(total, rng.choice([1, 2, 3, 7, 40]))))
            total -= sizes[-1]
        return sizes

    cases = []
    for _ in range(150):
        cases.append((partition(2 * rng.randint(1, 20)), None))
        total = rng.randint(1, 40)
        cases.append((partition(total), partition(total)))
    return cases


def ask(cases):
    """The helper's answer to every case, in one run of the binary: per case the runs as tuples and the batches' ranges."""
    text = "".join(",".join(map(str, s0)) + ("" if s1 is None else " " + ",".join(map(str, s1))) + "\n" for s0, s1 in cases)
    out = subprocess.run([CLI, "--io-test", "pair-runs", "-"], input=text, capture_output=True, text=True, check=True).stdout
    answers, runs, touch = [], [], {}
    for line in out.splitlines():
        word = line.split()
        if word[0] == "run":
            runs.append(tuple(int(w) for w in word[1:]))
        elif word[0] == "batch":
            touch[(int(word[1]), int(word[2]))] = (int(word[3]), int(word[4]))
        else:
            assert line == "#end 0", line
            answers.append((runs, touch))
            runs, touch = [], {}
    assert len(answers) == len(cases)
    return answers


def brute_force(s0, s1):
    """Maximal runs of pairs whose mates stay in one batch per side: (ia, ib, first_a, first_b, n_pairs, pair)."""
    where = [[(b, i) for b, n in enumerate(s) for i in range(n)] for s in (s0, s1 if s1 is not None else [])]
    if s1 is None:
        pairs = [(where[0][2 * j], where[0][2 * j + 1]) for j in range(len(where[0]) // 2)]
    else:
        pairs = list(zip(where[0], where[1]))
    runs = []
    for j, (a, b) in enumerate(pairs):
        if runs and runs[-1][:2] == (a[0], b[0]):
            runs[-1] = runs[-1][:4] + (runs[-1][4] + 1, runs[-1][5])
        else:
            runs.append((a[0], b[0], a[1], b[1], 1, j))
    return runs


def check(s0, s1, runs, touch):
    sizes = (s0, s0 if s1 is None else s1)
    n_pairs = sum(s0) // 2 if s1 is None else sum(s0)
    # every pair ordinal once and in order, each run inside one batch per side, with the stride of its input's form
    done = 0
    for ia, ib, first_a, first_b, stride, n, pair in runs:
        assert n >= 1 and pair == done
        assert stride in (1, 2) and (n == 1 or stride == (2 if s1 is None else 1))
        assert first_a + (n - 1) * stride < sizes[0][ia] and first_b + (n - 1) * stride < sizes[1][ib]
        done += n
    assert done == n_pairs
    # no two adjacent runs could be joined
    for r, s in zip(runs, runs[1:]):
        assert r[:2] != s[:2]
    # the same runs as the walk by brute force (which says where each starts)
    assert [r[:4] + r[5:] for r in runs] == brute_force(s0, s1)
    # the batches' ranges list exactly the runs with a read of the batch
    fb = 0 if s1 is None else 1
    expect = {}
    for k, r in enumerate(runs):
        for key in {(0, r[0]), (fb, r[1])}:
            expect.setdefault(key, []).append(k)
    assert set(touch) == {(0, i) for i in range(len(s0))} | ({(1, i) for i in range(len(s1))} if s1 is not None else set())
    for key, (begin, end) in touch.items():
        assert list(range(begin, end)) == expect[key], key


def test_cli_binary_is_built():
    assert os.path.exists(CLI), "make -C kbbq_amd/csrc builds kbbq_amd/kbbq"


def test_named_cases():
    cases = [(s, None) for s in INTERLEAVED] + TWO_FILES
    for (s0, s1), (runs, touch) in zip(cases, ask(cases)):
        check(s0, s1, runs, touch)


def test_what_the_runs_of_some_cases_are():
    """Spelled out, so that the helper and the brute force cannot be wrong together."""
    (a, _), (b, _), (c, tc), (d, td) = ask([([3, 3], None), ([1, 1], None), ([2, 1, 1, 2], None), ([4, 4], [3, 5])])
    assert a == [(0, 0, 0, 1, 2, 1, 0), (0, 1, 2, 0, 1, 1, 1), (1, 1, 1, 2, 2, 1, 2)]
    assert b == [(0, 1, 0, 0, 1, 1, 0)]
    assert c == [(0, 0, 0, 1, 2, 1, 0), (1, 2, 0, 0, 1, 1, 1), (3, 3, 0, 1, 2, 1, 2)]
    assert tc == {(0, 0): (0, 1), (0, 1): (1, 2), (0, 2): (1, 2), (0, 3): (2, 3)}
    assert d == [(0, 0, 0, 0, 1, 3, 0), (0, 1, 3, 0, 1, 1, 3), (1, 1, 0, 1, 1, 4, 4)]
    assert td == {(0, 0): (0, 2), (0, 1): (2, 3), (1, 0): (0, 1), (1, 1): (1, 3)}


def test_random_partitions():
    cases = random_cases()
    for (s0, s1), (runs, touch) in zip(cases, ask(cases)):
        check(s0, s1, runs, touch)


@pytest.mark.parametrize("args,text", [
    (["3"], " Error: --interleaved: an odd number of reads."),
    (["2,2,1"], " Error: --interleaved: an odd number of reads."),
    (["3", "4"], " Error: --in2: the files are not in step."),
    (["2,2", "2,1"], " Error: --in2: the files are not in step."),
])
def test_refusals(args, text):
    got = subprocess.run([CLI, "--io-test", "pair-runs"] + args, capture_output=True, text=True)
    assert got.returncode == 1 and got.stdout == ""
    lines = got.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith("[") and lines[0].endswith("]" + text), got.stderr
