// optimizer_kind_check.cpp -- host only, no device: the accessors that report which optimizer is active (optimizer_active,
// adam_is_active, lamb_is_active, lars_is_active, layerwise_active) for each of the container's five kinds.  The C handle API exposes
// only layerwise_active(), so tests/test_boundary_compile.py builds and runs this program instead.  The kind is assigned directly
// (the setters need a finalized container, that is a device): what is checked is the mapping from the kind to the accessors.
#include <cstdio>

#include "architectures.h"

namespace {
struct Probe : architectures::Sequential {
    using Kind = OptKind;
    void force(Kind k) { opt_kind = k; }
};
}  // namespace

int main() {
    using Kind = Probe::Kind;
    struct Row {
        Kind kind;
        const char* name;
        bool optimizer, adam, lamb, lars, layerwise;
    };
    const Row rows[] = {
        {Kind::kPlain, "plain", false, false, false, false, false}, {Kind::kSgdm, "sgdm", true, false, false, false, false},
        {Kind::kAdam, "adam", true, true, false, false, false},     {Kind::kLamb, "lamb", true, false, true, false, true},
        {Kind::kLars, "lars", true, false, false, true, true},
    };
    Probe net;
    int bad = net.optimizer_active() || net.adam_is_active() || net.lamb_is_active() || net.lars_is_active() || net.layerwise_active();
    if (bad) std::printf("a new container reports an optimizer\n");
    for (const Row& r : rows) {
        net.force(r.kind);
        const bool ok = net.optimizer_active() == r.optimizer && net.adam_is_active() == r.adam && net.lamb_is_active() == r.lamb &&
                        net.lars_is_active() == r.lars && net.layerwise_active() == r.layerwise;
        if (!ok) {
            std::printf("%s: optimizer %d adam %d lamb %d lars %d layerwise %d\n", r.name, net.optimizer_active(), net.adam_is_active(),
                        net.lamb_is_active(), net.lars_is_active(), net.layerwise_active());
            ++bad;
        }
    }
    net.force(Kind::kPlain);
    if (!bad) std::printf("ok\n");
    return bad ? 1 : 0;
}
