// devbuf_check.cpp -- csrc/dev_buf.h on the host (tests/test_devbuf_host.py): the allocation policy of ensure() and
// the ownership rules of DevBuf, against hip_shim.h's count of live blocks.  Exits non-zero at the first failure.
#include "../../rust-compression_amd/csrc/dev_buf.h"

#include <cstdio>
#include <type_traits>
#include <utility>

static_assert(!std::is_copy_constructible<DevBuf>::value, "a DevBuf is not copied");
static_assert(!std::is_copy_assignable<DevBuf>::value, "a DevBuf is not copied");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value,
              "a DevBuf moves without throwing");

static long live() { return hipshim::live_allocs().load(); }

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "devbuf_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                            \
        }                                                                        \
    } while (0)

struct Three {
    DevBuf a, b, c;
};

static int run()
{
    CHECK(live() == 0);
    {
        DevBuf b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(1000) == BZ_OK && b.p && b.cap == 1000 + 1000 / 8 + 256 && live() == 1);
        void *first = b.p;
        CHECK(b.ensure(b.cap) == BZ_OK && b.p == first && live() == 1); // within capacity: the same block
        CHECK(b.ensure(10) == BZ_OK && b.p == first && b.cap == 1000 + 1000 / 8 + 256);
        CHECK(b.as<char>() == static_cast<char *>(first));
        CHECK(b.ensure(5000) == BZ_OK && b.cap == 5000 + 5000 / 8 + 256 && live() == 1); // growth frees the old block
        static_cast<char *>(b.p)[b.cap - 1] = 1;
        hipshim::fail_next_mallocs() = 1; // the generous size is refused: the exact size is taken
        CHECK(b.ensure(20000) == BZ_OK && b.p && b.cap == 20000 && live() == 1);
        hipshim::fail_next_mallocs() = 2; // both refused
        CHECK(b.ensure(40000) == BZ_E_NOMEM && b.p == nullptr && b.cap == 0 && live() == 0);
        CHECK(hipshim::fail_next_mallocs() == 0);
        CHECK(b.ensure(64) == BZ_OK && live() == 1);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && live() == 0);
        b.release(); // (twice is harmless)
        CHECK(b.ensure(64) == BZ_OK && live() == 1);
    }
    CHECK(live() == 0); // leaving scope frees

    {
        DevBuf a;
        CHECK(a.ensure(100) == BZ_OK);
        void *pa = a.p;
        const size_t ca = a.cap;
        DevBuf m(std::move(a)); // move construction
        CHECK(m.p == pa && m.cap == ca && a.p == nullptr && a.cap == 0 && live() == 1);
        DevBuf t;
        CHECK(t.ensure(300) == BZ_OK && live() == 2);
        t = std::move(m); // move assignment into a buffer that holds a block: that block is freed
        CHECK(t.p == pa && t.cap == ca && m.p == nullptr && m.cap == 0 && live() == 1);
        DevBuf &self = t;
        t = std::move(self); // self-move
        CHECK(t.p == pa && t.cap == ca && live() == 1);
        static_cast<char *>(t.p)[0] = 1;
        DevBuf empty;
        t = std::move(empty); // an empty source empties the target
        CHECK(t.p == nullptr && t.cap == 0 && live() == 0);
    }
    CHECK(live() == 0);

    {
        Three s; // what an engine is: several buffers, an allocation that fails half way, one destructor
        CHECK(s.a.ensure(100) == BZ_OK);
        hipshim::fail_next_mallocs() = 2;
        CHECK(s.b.ensure(100) == BZ_E_NOMEM);
        CHECK(s.c.ensure(100) == BZ_OK && live() == 2);
    }
    CHECK(live() == 0);
    {
        Three *s = new Three;
        CHECK(s->a.ensure(1) == BZ_OK && s->b.ensure(2) == BZ_OK && s->c.ensure(3) == BZ_OK && live() == 3);
        delete s; // the buffers go with the delete
        CHECK(live() == 0);
    }
    return 0;
}

int main()
{
    const int rc = run();
    if (rc == 0) printf("ok\n");
    return rc;
}
