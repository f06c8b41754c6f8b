// stager_layout_check.cpp -- cnn_amd/csrc/stager_layout.h held to what include/cnn_amd.h documents, on the CPU: no device, no library.
// tests/test_stager_layout.py builds it with AddressSanitizer and UBSan and runs it.  For every kind, B in {1, 3, 8192} and, for the
// resident kind, levels in {1, 2, 14}: the parts of a slot's parameter block lie in the documented order, are 4-byte aligned and pairwise
// disjoint, their sizes sum to the block's, every size equals the header's formula -- written out HERE -- and the part predicate is the
// accessors' table.  Then the block is allocated and every part written through its offset: a part that ran past the block is the
// sanitizer's to find.
#include <cstdio>
#include <cstring>
#include <vector>

#include "stager_layout.h"

using namespace cnn_amd;

static int failures = 0;
#define CHECK(cond)                                                                                                  \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            ++failures;                                                                                              \
            std::printf("line %d: %s (kind %d, B %d, levels %d)\n", __LINE__, #cond, (int)s.kind, s.B, s.levels); \
        }                                                                                                            \
    } while (0)

static void check(StagerKind kind, int B, int levels) {
    StagerShape s;
    s.kind = kind;
    s.B = B;
    s.levels = levels;
    s.Hs = 9; s.Ws = 7; s.H = 5; s.W = 3;
    if (kind == StagerKind::U8) s.Hs = s.H, s.Ws = s.W;
    s.batch_bytes = kind == StagerKind::Raw ? 12345 : 0;
    const SlotLayout l = slot_layout(s);
    const size_t b = (size_t)B;
    const bool aug = kind == StagerKind::Aug, photo = kind == StagerKind::Photo, res = kind == StagerKind::Resident;

    // the accessors' table: matrices, fill | photo, normalize | indices, labels | levels
    CHECK(stager_has(s, StagerPart::Maps) == (aug || photo || res));
    CHECK(stager_has(s, StagerPart::Photo) == (photo || res));
    CHECK(stager_has(s, StagerPart::Indices) == res);
    CHECK(stager_has(s, StagerPart::Levels) == (res && levels > 1));
    CHECK(stager_has(s, StagerPart::LevelMaps) == (res && levels > 1));

    // include/cnn_amd.h: the sizes
    const size_t image = kind == StagerKind::Raw ? 12345 : res ? 0 : b * (size_t)s.Hs * (size_t)s.Ws * 3;
    const size_t param = aug ? b * 6 * 4 : photo ? b * 26 * 4 : res ? b * 4 + b * 26 * 4 + (levels > 1 ? b * 4 + b * 6 * 4 : 0) : 0;
    CHECK(l.image_bytes == image);
    CHECK(l.param_bytes == param);
    CHECK(l.out_bytes == (kind == StagerKind::Raw ? 0 : b * 3 * 5 * 3 * 4));
    CHECK(l.label_bytes == (res ? b * 4 : 0));

    // ... and the block: [B indices][B*6 maps][B*20 photo][B levels][B*6 level maps], the absent parts marked
    const size_t words[kStagerParts] = {1, 6, 20, 1, 6};
    const StagerPart order[kStagerParts] = {StagerPart::Indices, StagerPart::Maps, StagerPart::Photo, StagerPart::Levels, StagerPart::LevelMaps};
    size_t end = 0, sum = 0;
    for (int i = 0; i < kStagerParts; ++i) {
        const size_t off = l.offset[(int)order[i]], bytes = b * words[i] * 4;
        CHECK(stager_part_words(order[i]) == words[i]);
        if (!stager_has(s, order[i])) {
            CHECK(off == kNoPart);
            continue;
        }
        CHECK(off != kNoPart && off % 4 == 0);
        CHECK(off >= end);  // behind every part before it: in order, and disjoint from each of them
        CHECK(off + bytes <= l.param_bytes);
        end = off + bytes;
        sum += bytes;
    }
    CHECK(sum == l.param_bytes && end == l.param_bytes);
    if (res) CHECK(l.offset[(int)StagerPart::Indices] == 0 && l.offset[(int)StagerPart::Maps] == b * 4 && l.offset[(int)StagerPart::Photo] == b * 28);
    if (res && levels > 1) CHECK(l.offset[(int)StagerPart::Levels] == b * 108 && l.offset[(int)StagerPart::LevelMaps] == b * 112);
    if (aug || photo) CHECK(l.offset[(int)StagerPart::Maps] == 0);
    if (photo) CHECK(l.offset[(int)StagerPart::Photo] == b * 24);

    // every part written through its offset, each with its own byte: no part reaches another or leaves the block
    std::vector<unsigned char> block(l.param_bytes);
    for (int i = 0; i < kStagerParts; ++i)
        if (stager_has(s, order[i])) std::memset(block.data() + l.offset[(int)order[i]], i + 1, b * words[i] * 4);
    for (int i = 0; i < kStagerParts; ++i)
        if (stager_has(s, order[i])) {
            const unsigned char* p = block.data() + l.offset[(int)order[i]];
            CHECK(p[0] == i + 1 && p[b * words[i] * 4 - 1] == i + 1);
        }
}

// the layout is a constant expression
static_assert(slot_layout(StagerShape{StagerKind::Resident, 3, 8, 8, 5, 3, 2, 0}).param_bytes == 3 * (4 + 104 + 4 + 24), "resident block");
static_assert(kMaxDim == 8192 && kMaxLevels == 14 && kMapFloats == 6 && kPhotoFloats == 20, "limits");

int main() {
    const StagerKind kinds[] = {StagerKind::Raw, StagerKind::U8, StagerKind::Aug, StagerKind::Photo, StagerKind::Resident};
    const int batches[] = {1, 3, 8192}, levels[] = {1, 2, 14};
    for (StagerKind k : kinds)
        for (int B : batches)
            for (int L : levels)
                if (L == 1 || k == StagerKind::Resident) check(k, B, L);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
