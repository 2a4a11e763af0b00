"""CPU tests of the recalibration table file (kbbq_host_table_write / kbbq_host_table_read): a round trip of random sparse
histograms, the model trained from the loaded arrays, identical bytes from identical arguments, and every kind of
malformed file -- each made by editing one good file -- refused with KBBQ_EINVAL and the number of the offending line.
No GPU is touched."""
import numpy as np
import pytest

import common  # noqa: F401  (puts the repository root on sys.path)
from kbbq_amd import KbbqError
from kbbq_amd.engine import host_train, read_table, write_table

NQ = 256
EINVAL = -22


def sparse_cov(seed, n_rg, n_cycle):
    """Random sparse histograms: few cells are set, errors <= total, totals up to 2^63."""
    rng = np.random.RandomState(seed)
    cov = dict(R=n_rg, C=n_cycle, rg=np.zeros((n_rg, 2), np.uint64), q=np.zeros((n_rg, NQ, 2), np.uint64),
               cycle=np.zeros((n_rg, NQ, 2, n_cycle, 2), np.uint64), dinuc=np.zeros((n_rg, NQ, 16, 2), np.uint64))
    for key, share in (("rg", 0.7), ("q", 0.1), ("cycle", 0.02), ("dinuc", 0.05)):
        a = cov[key].reshape(-1, 2)
        n = max(1, int(len(a) * share))
        at = rng.choice(len(a), size=n, replace=False)
        # small counts (what a run gives, and what trains to a model that is not flat) and a few huge ones
        total = rng.randint(1, 100000, size=n).astype(np.uint64)
        huge = rng.rand(n) < 0.1
        total[huge] = (rng.randint(0, 1 << 31, size=int(huge.sum())).astype(np.uint64) << np.uint64(32)) | np.uint64(1)
        err = (total.astype(np.float64) * rng.rand(n) * 0.3).astype(np.uint64)
        a[at, 0] = np.minimum(err, total)
        a[at, 1] = total
    cov["cycle"][0, 30, 0, 0] = (1 << 63, 1 << 63)      # the largest count the tests ask for, errors == total
    cov["q"][n_rg - 1, 255] = (0, (1 << 63) - 1)
    return cov


CASES = {"one_cycle": (3, 1, ["lane1", "", "a b:c"]), "reads_151": (4, 151, ["", "A", "B.2", "rg with spaces"]), "fastq": (1, 151, [""])}


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_trip_and_model(case, tmp_path):
    n_rg, n_cycle, ids = CASES[case]
    cov = sparse_cov(len(case), n_rg, n_cycle)
    path = tmp_path / "t.tbl"
    write_table(path, cov, ids, k=32, seed=4242, total_bases=10 ** 12, command="kbbq --save-table t.tbl\tx\ny")
    got = read_table(path)
    assert got["R"] == n_rg and got["C"] == n_cycle and got["rg_ids"] == ids
    for key in ("rg", "q", "cycle", "dinuc"):
        assert got[key].dtype == np.uint64 and np.array_equal(got[key], cov[key]), key
    want_dq, got_dq = host_train(cov), host_train(got)
    for key in ("meanq", "rg", "q", "cycle", "dinuc"):
        assert np.array_equal(got_dq[key], want_dq[key]), key
    assert np.abs(want_dq["cycle"]).max() > 0      # (a model worth comparing)
    # only the cells that count are in the file, and the '#' lines are not data
    text = path.read_text()
    rows = [ln for ln in text.splitlines() if ln.split("\t")[0] in ("rg", "q", "cycle", "dinuc")]
    assert len(rows) == sum(int(np.count_nonzero(cov[k][..., 1])) for k in ("rg", "q", "cycle", "dinuc"))
    assert text.startswith("#kbbq-table 1\n") and text.endswith("end\t%d\n" % len(rows))
    stripped = tmp_path / "s.tbl"
    stripped.write_text("".join(ln + "\n" for i, ln in enumerate(text.splitlines()) if i == 0 or not ln.startswith("#")))
    assert np.array_equal(read_table(stripped)["cycle"], cov["cycle"])


def test_writing_twice_gives_identical_bytes(tmp_path):
    cov = sparse_cov(5, 2, 40)
    for name in ("a", "b"):
        write_table(tmp_path / name, cov, ["x", ""], k=21, seed=7, total_bases=123, command="kbbq in.bam")
    assert (tmp_path / "a").read_bytes() == (tmp_path / "b").read_bytes()


def test_writer_refuses_what_it_could_not_read_back(tmp_path):
    cov = sparse_cov(6, 2, 3)
    for ids in (["a", "a"], ["a\tb", "c"], ["a\n", "c"]):
        with pytest.raises(KbbqError) as ei:
            write_table(tmp_path / "w", cov, ids)
        assert ei.value.code == EINVAL
    cov["dinuc"][1, 7, 3] = (5, 4)
    with pytest.raises(KbbqError) as ei:
        write_table(tmp_path / "w", cov, ["a", "b"])
    assert ei.value.code == EINVAL


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """One good table as lines; with 3 read groups, 5 cycles and a known first row of every kind."""
    cov = sparse_cov(11, 3, 5)
    cov["cycle"][2, 40, 1, 4] = (3, 9)
    path = tmp_path_factory.mktemp("table") / "good.tbl"
    write_table(path, cov, ["g0", "", "g2"], k=32, seed=1, total_bases=1000, command="kbbq x")
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and read_table(path)["R"] == 3
    return lines[:-1]


def first(lines, word):
    return next(i for i, ln in enumerate(lines) if ln.split("\t")[0] == word)


def edits(lines):
    """name -> (edited lines or raw text, the 1-based line the reader must name)."""
    out = {}

    def put(name, at, new=None, insert=None):
        ls = list(lines)
        if insert is not None:
            ls.insert(at, insert)
        else:
            ls[at] = new
        out[name] = ("".join(ln + "\n" for ln in ls), at + 1)

    put("unknown_version", 0, "#kbbq-table 2")
    put("not_a_table", 0, "#something else")
    c = first(lines, "cycle")
    f = lines[c].split("\t")
    put("rg_index_out_of_range", c, "\t".join([f[0], "3"] + f[2:]))
    put("q_index_out_of_range", c, "\t".join(f[:2] + ["256"] + f[3:]))
    put("pair_index_out_of_range", c, "\t".join(f[:3] + ["2"] + f[4:]))
    put("cycle_index_out_of_range", c, "\t".join(f[:4] + ["5"] + f[5:]))
    put("huge_index", c, "\t".join(f[:4] + ["18446744073709551615"] + f[5:]))
    d = first(lines, "dinuc")
    g = lines[d].split("\t")
    put("dinuc_index_out_of_range", d, "\t".join(g[:3] + ["16"] + g[4:]))
    put("row_given_twice", c + 1, insert=lines[c])
    put("row_given_twice_far_apart", d, insert=lines[first(lines, "q")])
    put("errors_above_total", c, "\t".join(f[:5] + ["10", "9"]))
    put("not_a_number", c, "\t".join(f[:5] + ["1x", f[6]]))
    put("negative_number", c, "\t".join(f[:5] + ["-1", f[6]]))
    put("empty_number", c, "\t".join(f[:5] + ["", f[6]]))
    put("overflows_u64", c, "\t".join(f[:5] + ["1", "18446744073709551616"]))
    put("too_few_fields", c, "\t".join(f[:6]))
    put("too_many_fields", c, lines[c] + "\t1")
    put("unknown_record", c, "cycles" + lines[c][5:])
    put("bad_n_cycle", first(lines, "n_cycle"), "n_cycle\t0")
    put("read_groups_out_of_order", first(lines, "read_group") + 1, "read_group\t2\t")
    put("read_group_id_twice", first(lines, "read_group") + 2, "read_group\t2\tg0")
    put("text_after_end", len(lines), insert="rg\t0\t1\t2")
    good_text = "".join(ln + "\n" for ln in lines)
    # truncated: at a line boundary (no end line: named is the line that is missing), inside a line, and to nothing
    out["truncated_before_end"] = ("".join(ln + "\n" for ln in lines[:-1]), len(lines))
    out["truncated_in_rows"] = ("".join(ln + "\n" for ln in lines[:c + 3]), c + 4)
    out["truncated_inside_a_line"] = (good_text[:len(good_text) - 4], len(lines))
    out["truncated_inside_a_row"] = ("".join(ln + "\n" for ln in lines[:c]) + lines[c][:7], c + 1)
    out["end_count_wrong"] = ("".join(ln + "\n" for ln in lines[:c] + lines[c + 1:]), len(lines) - 1)
    out["empty_file"] = ("", 1)
    # more than 65534 read groups: the line of the 65535th
    rg0 = first(lines, "read_group")
    many = lines[:rg0] + ["read_group\t%d\tid%d" % (i, i) for i in range(65535)] + lines[rg0 + 3:]
    out["too_many_read_groups"] = ("".join(ln + "\n" for ln in many), rg0 + 65535)
    return out


EDIT_NAMES = ["unknown_version", "not_a_table", "rg_index_out_of_range", "q_index_out_of_range", "pair_index_out_of_range",
              "cycle_index_out_of_range", "huge_index", "dinuc_index_out_of_range", "row_given_twice", "row_given_twice_far_apart",
              "errors_above_total", "not_a_number", "negative_number", "empty_number", "overflows_u64", "too_few_fields", "too_many_fields",
              "unknown_record", "bad_n_cycle", "read_groups_out_of_order", "read_group_id_twice", "text_after_end", "truncated_before_end",
              "truncated_in_rows", "truncated_inside_a_line", "truncated_inside_a_row", "end_count_wrong", "empty_file", "too_many_read_groups"]


def test_every_edit_is_listed(good):
    assert sorted(edits(good)) == sorted(EDIT_NAMES)


@pytest.mark.parametrize("name", EDIT_NAMES)
def test_malformed_table_is_refused_with_its_line(name, good, tmp_path):
    text, line = edits(good)[name]
    path = tmp_path / "bad.tbl"
    path.write_text(text)
    with pytest.raises(KbbqError) as ei:
        read_table(path)
    assert ei.value.code == EINVAL
    assert "line %d:" % line in str(ei.value), str(ei.value)


def test_a_missing_file_is_an_error(tmp_path):
    with pytest.raises(KbbqError):
        read_table(tmp_path / "nope.tbl")
