"""The per-stream table of the device library (lsnet_amd/csrc/per_stream.h) on the host, without a GPU: the header has no HIP in
it, so a stand-alone driver with its own main() is compiled here with g++ under AddressSanitizer + UBSan and run as a child
process.  The driver supplies lsn::fail (the library's is in csrc/lib_state.hip) and prints one `ok <check>` line per check it
passed; a sanitizer report or a failed check ends it with a non-zero status."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = r'''
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace lsn {
static char g_err[256];
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace lsn
#include "per_stream.h"

struct Entry {
    int id;
    double payload[5];
};
static int g_inits = 0;
static char g_keys[32];   // 32 distinct addresses that stand for stream handles

#define REQUIRE(cond)                                                    \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __func__, __LINE__, #cond);     \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int make(lsn::PerStream<Entry> &t, const void *key, Entry **e)
{
    return t.get(key, "driver", e, [&](Entry &n) {
        n.id = ++g_inits;
        return 0;
    });
}

static int find_creates_nothing()
{
    lsn::PerStream<Entry> t;
    REQUIRE(t.find(&g_keys[0]) == nullptr);
    REQUIRE(t.find(nullptr) == nullptr);
    // the table is still empty: 16 other keys fit, and the key that was looked up is still unknown
    Entry *e = nullptr;
    for (int i = 1; i <= 16; ++i) REQUIRE(make(t, &g_keys[i], &e) == 0);
    REQUIRE(t.find(&g_keys[0]) == nullptr);
    return 0;
}

static int init_once_per_key()
{
    lsn::PerStream<Entry> t;
    g_inits = 0;
    Entry *a = nullptr, *b = nullptr, *c = nullptr;
    REQUIRE(make(t, &g_keys[0], &a) == 0 && g_inits == 1);
    REQUIRE(make(t, &g_keys[0], &b) == 0 && g_inits == 1 && a == b);
    REQUIRE(make(t, &g_keys[1], &c) == 0 && g_inits == 2 && c != a);
    REQUIRE(make(t, &g_keys[1], &b) == 0 && make(t, &g_keys[0], &b) == 0 && g_inits == 2);
    REQUIRE(t.find(&g_keys[0]) == a && t.find(&g_keys[1]) == c && a->id == 1 && c->id == 2);
    // the default stream is a key like any other
    REQUIRE(make(t, nullptr, &b) == 0 && g_inits == 3 && t.find(nullptr) == b);
    return 0;
}

static int seventeenth_is_refused()
{
    lsn::PerStream<Entry> t;
    g_inits = 0;
    Entry *e = nullptr;
    for (int i = 0; i < 16; ++i) REQUIRE(make(t, &g_keys[i], &e) == 0 && e && e->id == i + 1);
    lsn::g_err[0] = 0;
    REQUIRE(make(t, &g_keys[16], &e) == LSN_ERR_RUNTIME);
    REQUIRE(strcmp(lsn::g_err, "driver: more than 16 streams use the library") == 0);
    REQUIRE(e == nullptr && g_inits == 16 && t.find(&g_keys[16]) == nullptr);
    // the sixteen that are in keep working
    REQUIRE(make(t, &g_keys[7], &e) == 0 && e->id == 8 && g_inits == 16);
    return 0;
}

static int failed_init_leaves_the_slot_free()
{
    lsn::PerStream<Entry> t;
    Entry *e = nullptr;
    for (int i = 0; i < 15; ++i) REQUIRE(make(t, &g_keys[i], &e) == 0);
    int calls = 0;
    auto failing = [&](Entry &n) {
        ++calls;
        n.id = -1;   // (a half-made entry: the next attempt must not see it)
        return lsn::fail(-77, "init said no");
    };
    REQUIRE(t.get(&g_keys[15], "driver", &e, failing) == -77);
    REQUIRE(strcmp(lsn::g_err, "init said no") == 0 && calls == 1);
    REQUIRE(t.find(&g_keys[15]) == nullptr);
    // the last slot is still free: the same key succeeds now, with a fresh entry, and fills the table
    REQUIRE(t.get(&g_keys[15], "driver", &e, [&](Entry &n) { return n.id == 0 ? 0 : -1; }) == 0);
    REQUIRE(e != nullptr && t.find(&g_keys[15]) == e);
    REQUIRE(make(t, &g_keys[16], &e) == LSN_ERR_RUNTIME);
    return 0;
}

static int entries_keep_their_addresses()
{
    lsn::PerStream<Entry> t;
    Entry *at[16];
    for (int i = 0; i < 16; ++i) {
        REQUIRE(make(t, &g_keys[i], &at[i]) == 0);
        at[i]->payload[4] = 100.0 + i;
        for (int j = 0; j <= i; ++j) REQUIRE(t.find(&g_keys[j]) == at[j] && at[j]->payload[4] == 100.0 + j);
    }
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < i; ++j) REQUIRE(at[i] != at[j]);
    return 0;
}

int main()
{
    int bad = 0;
#define RUN(f)                          \
    do {                                \
        if (f()) bad = 1;               \
        else printf("ok %s\n", #f);     \
    } while (0)
    RUN(find_creates_nothing);
    RUN(init_once_per_key);
    RUN(seventeenth_is_refused);
    RUN(failed_init_leaves_the_slot_free);
    RUN(entries_keep_their_addresses);
    return bad;
}
'''
CHECKS = ['find_creates_nothing', 'init_once_per_key', 'seventeenth_is_refused', 'failed_init_leaves_the_slot_free',
          'entries_keep_their_addresses']


@pytest.fixture(scope='module')
def driver_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('per_stream')
    src = d / 'driver.cpp'
    src.write_text(DRIVER)
    exe = d / 'driver'
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', f'-I{os.path.join(ROOT, "lsnet_amd", "csrc")}', str(src), '-o', str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)


def test_driver_ends_clean(driver_run):
    assert driver_run.returncode == 0, driver_run.stdout + driver_run.stderr
    assert 'runtime error' not in driver_run.stderr and 'AddressSanitizer' not in driver_run.stderr, driver_run.stderr


@pytest.mark.parametrize('check', CHECKS)
def test_per_stream(driver_run, check):
    assert f'ok {check}' in driver_run.stdout.splitlines(), driver_run.stdout + driver_run.stderr


def test_header_has_no_hip():
    """The table is keyed by an opaque pointer and makes no HIP call: that is what lets it be tested here."""
    with open(os.path.join(ROOT, 'lsnet_amd', 'csrc', 'per_stream.h')) as f:
        code = [ln.split('//')[0] for ln in f]
    assert not any('hip' in ln.replace('lsnet_hip.h', '') for ln in code)
