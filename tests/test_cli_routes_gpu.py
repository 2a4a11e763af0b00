"""Every way through the `kbbq` command line writes the same bytes, for each of the three input formats.

The first scan (device reader, block-parallel host parsers, serial host readers) and the switches that keep or drop what it
leaves behind decide which of pass 4's six writers runs (kbbq_amd/csrc/kbbq_cli.cc: main(); the writers are cli_pass4.h's):

    cell                                         FASTQ                     BAM                       SAM
    {}                                           write_from_device_reader  write_from_device_reader  write_from_device_reader
    KBBQ_KEEP_TEXT=0                             (the same, file read again in pass 4)
    KBBQ_DEVICE_READER=0                         write_resident_fastq      write_resident_bam        write_resident_records
    KBBQ_DEVICE_READER=0 KBBQ_HOST_CACHE_MB=0    write_reparsed_fastq      write_serial              write_serial
    KBBQ_RESIDENT=0                              write_reparsed_fastq      write_serial              write_serial
    KBBQ_SERIAL_PARSE=1                          write_resident_fastq      write_resident_bam        write_resident_records
    KBBQ_SERIAL_PARSE=1 KBBQ_HOST_CACHE_MB=0     write_serial              write_serial              write_serial
    KBBQ_HOST_DEFLATE=1                          write_resident_records    write_resident_records    write_resident_records
    KBBQ_HOST_DEFLATE=1 KBBQ_RESIDENT=0          write_serial              write_serial              write_serial

One CLI run per cell; the yardstick is the default run of the same input."""
import gzip

import pytest

import common
from test_cli_gpu import bam_dataset, run_cli, write_fastq
from test_cli_sam_gpu import sam_dataset

pytestmark = pytest.mark.gpu

BASE_ENV = {"KBBQ_SEED": "7", "KBBQ_TIMING": "1", "KBBQ_READER_PIECE_KB": "64", "KBBQ_BATCH_READS": "700"}
SIZE = dict(genome_len=12000, coverage=20, read_len=100)      # about 2400 reads: several pieces, several batches
CELLS = [
    {},
    {"KBBQ_KEEP_TEXT": "0"},
    {"KBBQ_DEVICE_READER": "0"},
    {"KBBQ_DEVICE_READER": "0", "KBBQ_HOST_CACHE_MB": "0"},
    {"KBBQ_RESIDENT": "0"},
    {"KBBQ_SERIAL_PARSE": "1"},
    {"KBBQ_SERIAL_PARSE": "1", "KBBQ_HOST_CACHE_MB": "0"},
    {"KBBQ_HOST_DEFLATE": "1"},
    {"KBBQ_HOST_DEFLATE": "1", "KBBQ_RESIDENT": "0"},
]


def make_input(fmt, tmp):
    """the command line's arguments for one input of this format"""
    if fmt == "FASTQ":
        d = common.make_dataset(seed=83, **SIZE)
        names = ["read%d/%d" % (r // 2, 1 + (r & 1)) for r in range(len(d["off"]) - 1)]      # no RG: field: the device reader takes the file
        path = tmp / "in.fq"
        write_fastq(path, d, names)
        return ["-g", d["genome_len"], path]
    if fmt == "BAM":
        return ["--set-oq", bam_dataset(tmp, rg_header=True, seed=84, **SIZE)[2]]
    return ["--set-oq", sam_dataset(tmp, seed=85, **SIZE)[2]]


@pytest.fixture(scope="module")
def default_runs(tmp_path_factory):
    """format -> (arguments, decompressed output of the default run); each input is built and run once"""
    made = {}

    def get(fmt):
        if fmt not in made:
            args = make_input(fmt, tmp_path_factory.mktemp(fmt.lower()))
            rc, out, err = run_cli(args, BASE_ENV)
            assert rc == 0, err
            made[fmt] = (args, gzip.decompress(out))
        return made[fmt]
    return get


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "+".join("%s=%s" % kv for kv in sorted(c.items())) or "default")
@pytest.mark.parametrize("fmt", ["FASTQ", "BAM", "SAM"])
def test_cli_every_route_writes_the_default_run_s_bytes(default_runs, fmt, cell):
    args, want = default_runs(fmt)
    assert len(want) > 3 * (64 << 10)
    rc, out, err = run_cli(args, dict(BASE_ENV, **cell))
    assert rc == 0, err
    assert gzip.decompress(out) == want
    assert ((fmt + " reader on the GPU") in err) == (cell in ({}, {"KBBQ_KEEP_TEXT": "0"})), err
    assert ("one scan" in err) == (cell == {}), err
