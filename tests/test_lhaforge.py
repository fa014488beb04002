"""The LHA archive forge (tests/lhaforge.py) before anything reads its archives: the fixture is what --regen made, every case
meets the targets it claims, REQUIRED is met in full, and the forge's own CRC-16 is CRC-16/ARC."""
import lhaforge as F


def test_crc16_is_crc16_arc():
    assert F.crc16(b"123456789") == 0xBB3D and F.crc16(b"") == 0
    assert F.crc16_table(b"123456789") == 0xBB3D
    data = bytes(range(256)) * 3 + b"tail"
    assert F.crc16_table(data) == F.crc16(data)
    assert F.crc16(data[100:], F.crc16(data[:100])) == F.crc16(data)


def test_fixture_is_what_regen_made():
    committed = F.load()
    fresh = F.base_cases()
    assert [c["name"] for c in committed] == [c["name"] for c in fresh]
    for c, f in zip(committed, fresh):
        assert {k: v for k, v in c.items() if k not in ("sha256", "hits")} == f, c["name"]
        assert c["sha256"] == F.digest(c), c["name"]


def test_every_case_hits_what_it_claims_and_required_is_met():
    got = set()
    for c in F.load():
        h = F.hits(c)
        assert h == c["hits"], c["name"]
        assert set(h) & F.REQUIRED, "%s alone hits no required target" % c["name"]
        got |= set(h)
    assert F.REQUIRED <= got, sorted(F.REQUIRED - got)


def test_families_and_sizes():
    cases = F.load()
    assert {c["family"] for c in cases} == set("LMCFPS")
    for c in cases:
        a = F.build(c)
        assert len(a.data) < 200_000 and all(len(p) <= 3 * F.PART + 5 for p in a.plains), c["name"]
        e = a.expect()
        assert len(e) == a.listed == len(F.index(a.data)[0])
        # each fault leaves its neighbours clean with their bytes
        if c["family"] == "F":
            assert sum(v == F.OK and len(b) > 0 for b, v in e) >= 2, c["name"]


def test_level_2_header_size_never_ends_in_a_zero_byte():
    for c in F.load():
        a = F.build(c)
        for m in F.index(a.data)[0]:
            assert a.data[m["header_off"]] != 0
