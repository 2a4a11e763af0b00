"""CPU tests of the quality report file (kbbq_host_report_write / kbbq_host_report_read): a round trip of a random
consistent report with and without `observed` rows, identical bytes from identical arguments, the empty read-group id, and
every refusal -- each made by editing one good file -- with KBBQ_EINVAL and the number of the offending line.  No GPU is touched."""
import numpy as np
import pytest

import common  # noqa: F401  (puts the repository root on sys.path)
import plain_report_ref as ref
from kbbq_amd import KbbqError
from kbbq_amd.engine import read_report, write_report

NQ = 256
EINVAL = -22


def random_report(seed, n_rg, n_cycle, n_reads=300):
    """A report that a run could have made: the numpy definition over random reads (every read group's totals agree)."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, n_cycle + 1, size=n_reads)
    off = np.zeros(n_reads + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    nb = int(off[-1])
    qual = rng.randint(0, 256, size=nb).astype(np.uint8)
    out = rng.randint(0, 94, size=nb).astype(np.uint8)
    return ref.report(qual, out, off, rng.randint(0, n_rg, size=n_reads), rng.randint(0, 2, size=n_reads), n_rg, n_cycle)


def observed_cov(seed, n_rg, n_cycle):
    rng = np.random.RandomState(seed)
    cov = dict(R=n_rg, C=n_cycle, rg=np.zeros((n_rg, 2), np.uint64), q=np.zeros((n_rg, NQ, 2), np.uint64),
               cycle=np.zeros((n_rg, NQ, 2, n_cycle, 2), np.uint64), dinuc=np.zeros((n_rg, NQ, 16, 2), np.uint64))
    at = rng.rand(n_rg, NQ) < 0.2
    total = rng.randint(1, 1 << 40, size=(n_rg, NQ)).astype(np.uint64)
    cov["q"][..., 1] = np.where(at, total, 0)
    cov["q"][..., 0] = np.where(at, total // np.uint64(7), 0)
    cov["q"][n_rg - 1, 255] = ((1 << 63) - 1, (1 << 63) - 1)
    return cov


CASES = {"one_cycle": (3, 1, ["lane1", "", "a b:c"]), "reads_151": (4, 151, ["", "A", "B.2", "rg with spaces"]), "fastq": (1, 151, [""])}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("with_observed", [False, True])
def test_round_trip(case, with_observed, tmp_path):
    n_rg, n_cycle, ids = CASES[case]
    rep = random_report(len(case), n_rg, n_cycle)
    rep["above_maxq"] = 12345
    cov = observed_cov(3, n_rg, n_cycle) if with_observed else None
    path = tmp_path / "r.txt"
    write_report(path, rep, ids, observed=cov, k=32, seed=4242, total_bases=10 ** 12, command="kbbq --report r.txt\tx\ny")
    got = read_report(path)
    assert got["R"] == n_rg and got["C"] == n_cycle and got["rg_ids"] == ids and got["above_maxq"] == 12345      # the empty id is a value
    for key in ("transfer", "cycle"):
        assert got[key].dtype == np.uint64 and np.array_equal(got[key], rep[key]), key
    assert np.array_equal(got["observed"], cov["q"] if with_observed else np.zeros((n_rg, NQ, 2), np.uint64))
    # only the cells that count are in the file, and the '#' lines are not data
    text = path.read_text()
    rows = [ln for ln in text.splitlines() if ln.split("\t")[0] in ("transfer", "cycle", "observed")]
    want_rows = int(np.count_nonzero(rep["transfer"])) + int(np.count_nonzero(rep["cycle"][..., 0])) + (int(np.count_nonzero(cov["q"][..., 1])) if with_observed else 0)
    assert len(rows) == want_rows
    assert text.startswith("#kbbq-report 1\n") and text.endswith("above_maxq\t12345\nend\t%d\n" % len(rows))
    people = [ln for ln in text.splitlines() if ln.startswith("#group\t")]
    assert len(people) == n_rg
    f = people[0].split("\t")
    bases0 = int(rep["transfer"][0].sum())
    assert f[1:4] == ["0", "bases", str(bases0)]
    assert f[5] == "%.4f" % (int(rep["cycle"][0, :, :, 1].sum()) / bases0) and f[7] == "%.4f" % (int(rep["cycle"][0, :, :, 2].sum()) / bases0)
    assert int(f[9]) == bases0 - int(sum(rep["transfer"][0, q, q] for q in range(94)))
    assert "#command\tkbbq --report r.txt\tx y" in text
    stripped = tmp_path / "s.txt"
    stripped.write_text("".join(ln + "\n" for i, ln in enumerate(text.splitlines()) if i == 0 or not ln.startswith("#")))
    assert np.array_equal(read_report(stripped)["cycle"], rep["cycle"])


def test_writing_twice_gives_identical_bytes(tmp_path):
    rep, cov = random_report(5, 2, 40), observed_cov(5, 2, 40)
    for name in ("a", "b"):
        write_report(tmp_path / name, rep, ["x", ""], observed=cov, k=21, seed=7, total_bases=123, command="kbbq in.bam")
    assert (tmp_path / "a").read_bytes() == (tmp_path / "b").read_bytes()


def test_writer_refuses_what_it_could_not_read_back(tmp_path):
    rep = random_report(6, 2, 30)
    for ids in (["a", "a"], ["a\tb", "c"], ["a\n", "c"]):
        with pytest.raises(KbbqError) as ei:
            write_report(tmp_path / "w", rep, ids)
        assert ei.value.code == EINVAL
    for key, at, value in (("cycle", (1, 0, 3, 0), 1 << 20), ("cycle", (0, 1, 2, 2), 1 << 40), ("transfer", (1, 200, 93), 1 << 30)):
        bad = dict(rep, transfer=rep["transfer"].copy(), cycle=rep["cycle"].copy())
        bad[key][at] += np.uint64(value)
        with pytest.raises(KbbqError) as ei:
            write_report(tmp_path / "w", bad, ["a", "b"])
        assert ei.value.code == EINVAL
    with pytest.raises(KbbqError) as ei:
        write_report(tmp_path / "no" / "such" / "dir", rep, ["a", "b"])
    assert ei.value.code == -5


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """One good report as lines: 3 read groups, 5 cycles, observed rows."""
    rep, cov = random_report(11, 3, 5, n_reads=60), observed_cov(11, 3, 5)
    path = tmp_path_factory.mktemp("report") / "good.txt"
    write_report(path, rep, ["g0", "", "g2"], observed=cov, k=32, seed=1, total_bases=1000, command="kbbq x")
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and read_report(path)["R"] == 3
    return lines[:-1]


def first(lines, word, rg=None):
    return next(i for i, ln in enumerate(lines) if ln.split("\t")[0] == word and (rg is None or ln.split("\t")[1] == str(rg)))


def edits(lines):
    """name -> (the edited text, the 1-based line the reader must name)."""
    out = {}

    def put(name, at, new=None, insert=None, names=None):
        ls = list(lines)
        if insert is not None:
            ls.insert(at, insert)
        else:
            ls[at] = new
        out[name] = ("".join(ln + "\n" for ln in ls), (at if names is None else names) + 1)

    def fields(at, **change):
        f = lines[at].split("\t")
        for i, v in change.items():
            f[int(i[1:])] = str(v)
        return "\t".join(f)

    t, c, o, end = first(lines, "transfer"), first(lines, "cycle"), first(lines, "observed"), first(lines, "end")
    tf, cf = lines[t].split("\t"), lines[c].split("\t")
    put("q_out_above_93", t, fields(t, f3=94))
    put("q_in_out_of_range", t, fields(t, f2=256))
    put("read_group_out_of_range", t, fields(t, f1=3))
    put("pair_out_of_range", c, fields(c, f2=2))
    put("cycle_out_of_range", c, fields(c, f3=5))
    put("sum_in_above_255_times_bases", c, fields(c, f5=255 * int(cf[4]) + 1))
    put("sum_out_above_93_times_bases", c, fields(c, f6=93 * int(cf[4]) + 1))
    put("observed_errors_above_total", o, fields(o, f3=int(lines[o].split("\t")[4]) + 1))
    put("transfer_row_twice", t + 1, insert=lines[t])
    put("cycle_row_twice", c + 1, insert=lines[c])
    put("observed_row_twice", o + 1, insert=lines[o])
    put("zero_bases", t, fields(t, f4=0))
    put("not_a_number", t, fields(t, f4="12x"))
    put("overflow", t, fields(t, f4=1 << 64))
    put("too_few_fields", c, "\t".join(cf[:-1]))
    put("unknown_record", t, "transfers\t0\t0\t0\t1")
    # a read group whose transfer total differs from its cycle total: found where the totals are complete, at the end line
    put("totals_differ", t, fields(t, f4=int(tf[4]) + 1), names=end)
    put("end_count_wrong", end, "end\t%d" % (int(lines[end].split("\t")[1]) + 1))
    put("text_after_end", end + 1, insert="transfer\t0\t0\t0\t1")
    put("above_maxq_twice", end, insert=lines[end - 1])
    put("row_after_above_maxq", end, insert="observed\t0\t1\t0\t5")
    put("read_group_out_of_order", first(lines, "read_group") + 1, "read_group\t2\tx")
    put("read_group_id_twice", first(lines, "read_group") + 1, "read_group\t1\tg0")
    put("n_cycle_zero", first(lines, "n_cycle"), "n_cycle\t0")
    put("version", 0, "#kbbq-report 2")
    put("not_a_report", 0, "#kbbq-table 1")
    missing_end = [ln for ln in lines if not ln.startswith("end\t")]
    out["missing_end"] = ("".join(ln + "\n" for ln in missing_end), len(missing_end) + 1)
    out["cut_inside_a_line"] = ("".join(ln + "\n" for ln in lines)[:-3], len(lines))
    out["empty"] = ("", 1)
    return out


EDITS = ["q_out_above_93", "q_in_out_of_range", "read_group_out_of_range", "pair_out_of_range", "cycle_out_of_range", "sum_in_above_255_times_bases",
         "sum_out_above_93_times_bases", "observed_errors_above_total", "transfer_row_twice", "cycle_row_twice", "observed_row_twice", "zero_bases",
         "not_a_number", "overflow", "too_few_fields", "unknown_record", "totals_differ", "end_count_wrong", "text_after_end", "above_maxq_twice",
         "row_after_above_maxq", "read_group_out_of_order", "read_group_id_twice", "n_cycle_zero", "version", "not_a_report", "missing_end",
         "cut_inside_a_line", "empty"]


@pytest.mark.parametrize("name", EDITS)
def test_reader_refuses_and_names_the_line(good, name, tmp_path):
    all_edits = edits(good)
    assert sorted(all_edits) == sorted(EDITS)
    text, line = all_edits[name]
    path = tmp_path / "bad.txt"
    path.write_text(text)
    with pytest.raises(KbbqError) as ei:
        read_report(path)
    assert ei.value.code == EINVAL
    assert "line %d:" % line in str(ei.value), (name, str(ei.value))


def test_a_file_cut_at_any_line_boundary_is_refused(good, tmp_path):
    path = tmp_path / "cut.txt"
    for n in range(len(good)):
        path.write_text("".join(ln + "\n" for ln in good[:n]))
        with pytest.raises(KbbqError) as ei:
            read_report(path)
        assert ei.value.code == EINVAL and "line %d:" % (n + 1 if n else 1) in str(ei.value), (n, str(ei.value))
    path.write_text("".join(ln + "\n" for ln in good))
    assert read_report(path)["R"] == 3


def test_a_missing_file_is_an_error(tmp_path):
    with pytest.raises(KbbqError):
        read_report(tmp_path / "nothing")
