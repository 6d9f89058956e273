"""`tracy_amd_cli basecall --batch manifest.tsv -d 0`: the files read once into one buffer, then tracyhip_read_traces ->
tracyhip_basecall_traces -> tracyhip_render_traces on the device (fasta / fastq written by the host from the device's basecalls).  The
manifest of tests/test_cli_basecall_batch.py -- ABIF and SCF, a file that is no trace, a missing one, one whose trims take all of it --
with -f tsv / json / fastq and -t 0 / -t 2: `--batch -d 0`, `--batch` without -d and the one-file command per line must write identical
files and the same messages for the bad lines."""
import pytest

from test_cli_basecall_batch import FORMS, check_batch, expected, traces  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt,trim", FORMS)
def test_batch_on_the_device_equals_the_one_file_command(traces, expected, tmp_path, fmt, trim):  # noqa: F811
    check_batch(traces, str(tmp_path), fmt, trim, ["-d", "0"], expected[(fmt, trim)])
    check_batch(traces, str(tmp_path), fmt, trim, ["--threads", "1"], expected[(fmt, trim)])


def test_the_device_answers_the_good_lines_itself(traces, tmp_path):  # noqa: F811
    """the nine good lines never take the one-file chain: the command says how many traces the device read, basecalled and wrote.  A
    stringency above 9 is what the device does not take (the one-file command calls trimTrace unclamped): every line goes to the host."""
    from test_cli_basecall_batch import batch
    for fmt in ("tsv", "json", "fasta"):
        p, _ = batch(traces, str(tmp_path / fmt), fmt, "0", ["-d", "0"])
        assert p.returncode == 2 and "Device: 9 of 12 traces read, basecalled and written" in p.stdout, p.stdout
    p, _ = batch(traces, str(tmp_path / "host"), "tsv", "0", [])
    assert "Device:" not in p.stdout
    p, _ = batch(traces, str(tmp_path / "t12"), "tsv", "12", ["-d", "0"])
    assert "Device:" not in p.stdout
