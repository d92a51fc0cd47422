"""Host side of the encoders' per-stream inputs, no GPU: every stream's own frame bytes (what a mixed call's
rows and strides are sized by), the new entry point and flag in the headers and the binding, the file
encoders' option checks with the flag set, and the ABI version, which the suite's host tests pin to 2 (a
function was only added)."""
import re
from pathlib import Path

from in_cwave_amd import abi
from in_cwave_amd import lib as L

ROOT = Path(__file__).resolve().parent.parent


def test_a_streams_own_frame_bytes():
    """what a mixed call's rows are sized by: every stream's own FB, the widest holding each narrower one"""
    expect = {abi.FMT_CW_F64: 16, abi.FMT_CW_I16: 4, abi.FMT_CW_I16_F32: 6, abi.FMT_CW_F32: 8}
    for cw, cb in expect.items():
        for ch, nc in ((1, 1), (2, 2), (3, 2)):
            assert L.cwave_frame_bytes(cw, ch) == cb * nc
        assert L.cwave_frame_bytes(cw, 2) == 2 * L.cwave_frame_bytes(cw, 1)
        assert L.cwave_frame_bytes(cw, 0) == 0
    assert L.cwave_frame_bytes(abi.FMT_I16, 2) == 0 and L.cwave_frame_bytes(abi.FMT_CW_F32 + 1, 2) == 0


def test_entry_points_and_flag():
    lib = L.load()
    assert lib.icw_enable_stream_encode(None, 1) == abi.EINVAL
    assert lib.icw_enable_stream_encode(None, 0) == abi.EINVAL
    icw_h = (ROOT / "include" / "icw.h").read_text()
    reader_h = (ROOT / "include" / "icw_reader.h").read_text()
    assert "int icw_enable_stream_encode(icw_ctx *ctx, int on);" in icw_h
    assert int(re.search(r"#define ICW_ENC_MERGE_INPUTS (\d+)", reader_h).group(1)) == abi.ENC_MERGE_INPUTS == 1
    assert lib.icw_abi_version() == int(re.search(r"#define ICW_ABI_VERSION (\d+)", icw_h).group(1)) == 2


def test_file_encoders_with_the_flag_still_check_their_options(tmp_path):
    never = tmp_path / "never.cwave"
    rc, _, _, _ = L.cwave_encode_files_iir([tmp_path / "none.wav"], [never], hilbert_type=6, merge_inputs=True)
    assert rc == abi.EINVAL and not never.exists()
    rc, _, _, _ = L.cwave_encode_files([tmp_path / "none.wav"], [never], 31, merge_inputs=True)
    assert rc == abi.EINVAL and not never.exists()
    # no file accepted: nothing to merge, no context, no device
    rc, st, status, _ = L.cwave_encode_files_iir([tmp_path / "none.wav"], [never], merge_inputs=True)
    assert rc == abi.EINVAL and status == [abi.EINVAL] and st.n_groups == 0 and st.n_files == 0
