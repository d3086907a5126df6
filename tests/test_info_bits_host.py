"""vh_result_info.reserved on the CPU: the composer of viyadb_amd/csrc/vhh_info.h against the numerals the bits had before they had names.
No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_composer_equals_the_numerals(tmp_path):
    """tests/info_bits_host.cc carries the expression QueryBuild::launch() held in numerals, with the two rewrites for the pre-built plane
    readers behind it, and the select's. It asserts vh_info_compose equal to it over every combination of the struct's 27 booleans at
    4-byte records (2^27 cases), over records of 0, 1, 2, 4 .. 64 bytes times every combination of packed / packed_bits /
    packed_compressed / plane_agg / sliced_prebuilt with the other inputs all false and all true; vh_info_select over its 8 inputs;
    vh_info_rec_bytes over the 8 codes with bit 3 set and clear. A stand-alone program built with -O2 -fsanitize=undefined alone: under
    AddressSanitizer at -O1 the 2^27 cases take 8.5 s on a fast core and twice that on a slower one, with UBSan alone 3.3 s; the code
    under test allocates nothing and indexes nothing, so what UBSan watches (the shifts, the booleans' values) is what can go wrong."""
    exe = tmp_path / "info_bits_host"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "viyadb_amd", "csrc"),
                    os.path.join(ROOT, "tests", "info_bits_host.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 4 and all(line.endswith(": ok") for line in lines), run.stdout
