// The count / fill protocol of csrc/asr_pending.h on the CPU: a stand-alone program, built with the host compiler and
// -fsanitize=address,undefined by tests/test_pending_protocol.py.  Exit status 0 and "ok" when every statement holds.
#include <cstdio>
#include <cstdlib>

#include "../adaptive-surface-reconstruction_amd/csrc/asr_pending.h"

#define REQUIRE(expr)                                                         \
    do {                                                                      \
        if (!(expr)) {                                                        \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #expr); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

int main() {
    const PendingOp A = PendingOp::Contour, B = PendingOp::PointsMerge;
    uint64_t generation = 7;  // the scratch arena's; bumped by whatever recycles it
    Pending p;

    REQUIRE(!pending_claim(p, A, generation));  // a fresh context has nothing to fill

    // commit -> claim succeeds once
    pending_begin(p);
    pending_commit(p, A, generation);
    REQUIRE(pending_claim(p, A, generation));
    REQUIRE(!pending_claim(p, A, generation));

    // commit -> the arena is recycled -> claim fails, and stays failed at the old generation
    pending_begin(p);
    pending_commit(p, A, generation);
    ++generation;
    REQUIRE(!pending_claim(p, A, generation));
    REQUIRE(!pending_claim(p, A, generation - 1));

    // commit A -> claim B fails, and A is gone
    pending_begin(p);
    pending_commit(p, A, generation);
    REQUIRE(!pending_claim(p, B, generation));
    REQUIRE(!pending_claim(p, A, generation));

    // a count that began and did not succeed leaves nothing, not even the count before it
    pending_begin(p);
    pending_commit(p, A, generation);
    pending_begin(p);
    REQUIRE(!pending_claim(p, A, generation));
    pending_begin(p);
    REQUIRE(!pending_claim(p, B, generation));

    // a later commit replaces an earlier one, whatever the operator
    pending_begin(p);
    pending_commit(p, A, generation);
    pending_begin(p);
    pending_commit(p, B, generation);
    REQUIRE(!pending_claim(p, A, generation));
    pending_begin(p);
    pending_commit(p, A, generation);
    ++generation;
    pending_begin(p);
    pending_commit(p, A, generation);
    REQUIRE(pending_claim(p, A, generation));

    // every operator, and None never
    for (int op = (int)PendingOp::MultiRadiusSearch; op <= (int)PendingOp::PointsMerge; ++op) {
        pending_begin(p);
        pending_commit(p, (PendingOp)op, generation);
        REQUIRE(pending_claim(p, (PendingOp)op, generation));
    }
    pending_begin(p);
    REQUIRE(!pending_claim(p, PendingOp::None, generation));
    pending_commit(p, PendingOp::None, generation);
    REQUIRE(!pending_claim(p, PendingOp::None, generation));

    // the slots of a context and of its auxiliary context are independent
    Pending aux;
    pending_commit(p, A, generation);
    pending_begin(aux);
    REQUIRE(!pending_claim(aux, A, generation));
    REQUIRE(pending_claim(p, A, generation));

    puts("ok");
    return 0;
}
