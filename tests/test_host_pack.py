"""pack_pair (csrc/orbx_pack.hpp), the host packer of the two-frame entry points (no GPU).

A stand-alone C++ program, built with AddressSanitizer and UBSan where their runtimes are installed, packs two
sources into a destination of exactly 2 * cap elements and compares every byte with a direct expectation: a's
elements at 0, b's at cap, the fill byte everywhere else, a NULL source copying nothing whatever its count.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb-slam-_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <memory>
#include "orbx_pack.hpp"

template <size_t S>
struct Elem {
    unsigned char b[S];
};

static long g_cases = 0, g_bad = 0;

// sources of exactly n elements and a destination of exactly 2 * cap, all on the heap: an overrun by one
// byte on either side is the sanitizer's to report
template <size_t S>
void run(size_t n1, size_t n2, size_t cap, bool null_a, bool null_b, int fill)
{
    typedef Elem<S> E;
    std::unique_ptr<E[]> a(new E[n1]), b(new E[n2]), dst(new E[2 * cap]);
    for (size_t i = 0; i < n1 * S; ++i) reinterpret_cast<unsigned char*>(a.get())[i] = (unsigned char)(1 + i % 100);
    for (size_t i = 0; i < n2 * S; ++i) reinterpret_cast<unsigned char*>(b.get())[i] = (unsigned char)(101 + i % 100);
    unsigned char* out = reinterpret_cast<unsigned char*>(dst.get());
    for (size_t i = 0; i < 2 * cap * S; ++i) out[i] = 0xA5;   // neither fill byte, nor a source byte
    const E* pa = null_a ? nullptr : a.get();
    const E* pb = null_b ? nullptr : b.get();
    if (fill == 0) orbx::pack_pair(dst.get(), cap, pa, n1, pb, n2);   // the default fill
    else orbx::pack_pair(dst.get(), cap, pa, n1, pb, n2, fill);
    for (size_t j = 0; j < 2 * cap * S; ++j) {
        const size_t frame = j / (cap * S), off = j % (cap * S);
        const bool copied = frame == 0 ? (!null_a && off < n1 * S) : (!null_b && off < n2 * S);
        const unsigned char want = !copied ? (unsigned char)fill
                                           : frame == 0 ? (unsigned char)(1 + off % 100) : (unsigned char)(101 + off % 100);
        if (out[j] != want) {
            if (!g_bad)
                std::printf("first mismatch: size %zu n1 %zu n2 %zu cap %zu null %d%d fill %d byte %zu: %d, want %d\n", S,
                            n1, n2, cap, (int)null_a, (int)null_b, fill, j, (int)out[j], (int)want);
            ++g_bad;
        }
    }
    ++g_cases;
}

template <size_t S>
void all()
{
    static_assert(sizeof(Elem<S>) == S, "element size");
    const size_t shapes[6][3] = {{0, 0, 1}, {0, 3, 3}, {3, 0, 3}, {3, 3, 3}, {1, 4, 4}, {4, 1, 4}};
    for (const auto& s : shapes)
        for (int nulls = 0; nulls < 4; ++nulls)
            for (int fill : {0, 0xFF}) run<S>(s[0], s[1], s[2], nulls & 1, nulls & 2, fill);
}

int main()
{
    all<1>();
    all<4>();
    all<28>();   // orbx_keypoint
    all<32>();   // a descriptor
    all<48>();   // orbm_map_point
    std::printf("%ld %ld\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
"""


def _sanitizer_flags(tmp):
    """-fsanitize=address,undefined where a program built with it links and runs, else nothing."""
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    exe = os.path.join(tmp, "probe")
    try:
        subprocess.check_call(["g++"] + flags + [src, "-o", exe], stderr=subprocess.DEVNULL)
        subprocess.check_call([exe])
    except (OSError, subprocess.CalledProcessError):
        return []
    return flags


def test_pack_pair_every_byte(tmp_path):
    src = str(tmp_path / "pack_test.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM)
    exe = str(tmp_path / "pack_test")
    flags = _sanitizer_flags(str(tmp_path))
    print("sanitizer flags:", flags)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    cases, bad = map(int, r.stdout.split()[-2:])
    assert cases == 5 * 6 * 4 * 2 and bad == 0
