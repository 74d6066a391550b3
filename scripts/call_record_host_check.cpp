// Host-side sanitizer check of the call record (include/mvhmr_unproject.h): fills records of every family, placing and kind,
// asks the workspace query and the named queries, and makes launching calls the library refuses before any launch (null features, a
// malformed record).  No GPU is needed and nothing is launched.  Build capi.hip's host code under the sanitizers together with this file
// and link the library's other objects as they are (from multiviewhmr_amd/csrc, after `python -m multiviewhmr_amd.build`):
//   F="--offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I../../include -I."
//   hipcc $F -c capi.hip -o /tmp/capi_san.o && hipcc $F -x c++ -c ../../scripts/call_record_host_check.cpp -o /tmp/check_san.o &&
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/capi_san.o /tmp/check_san.o $(ls ../lib/*.o | grep -v /capi.o) -o /tmp/check &&
//   /tmp/check
#include <stdio.h>
#include <string.h>

#include "mvhmr_unproject.h"

static int failures = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) {                                                           \
            printf("line %d: %s  [%s]\n", __LINE__, #cond, mvhmr_last_error());  \
            failures++;                                                          \
        }                                                                        \
    } while (0)

int main()
{
    mvhmr_unproject_desc d;
    memset(&d, 0, sizeof(d));
    d.abi_version = MVHMR_ABI_VERSION;
    d.batch = 2, d.views = 4, d.channels = 8, d.feat_h = 24, d.feat_w = 20, d.vol_x = 8, d.vol_y = 6, d.vol_z = 5;
    d.method = MVHMR_AGG_MEAN;
    const double position[3] = {-1, -1, -1}, sides[3] = {2, 2, 2};
    float dummy[64] = {0};                        // host memory behind every pointer the refused calls are handed (none is read)
    int calls = 0;
    for (int family = MVHMR_FAMILY_PLAIN; family <= MVHMR_FAMILY_MOMENTS; family++)
        for (int placing = MVHMR_PLACING_TENSOR; placing <= MVHMR_PLACING_CUBOID; placing++)
            for (int det = 0; det < 2; det++) {
                mvhmr_unproject_call c;
                memset(&c, 0, sizeof(c));
                c.struct_size = sizeof(c);
                c.family = family;
                c.placing = placing;
                c.deterministic = det;
                c.volumes = 3;
                const size_t need[3] = {mvhmr_unproject_call_workspace_bytes(&d, &c, MVHMR_CALL_FORWARD),
                                        mvhmr_unproject_call_workspace_bytes(&d, &c, MVHMR_CALL_BACKWARD),
                                        mvhmr_unproject_call_workspace_bytes(&d, &c, MVHMR_CALL_GEOMETRY)};
                EXPECT(need[0] > 0 && need[1] >= need[0] && need[2] > 0);
                c.coords = c.rot = c.center = c.proj = dummy;
                c.position = position, c.sides = sides;
                c.grad_out = c.out = c.grad_features = c.grad_proj = dummy;
                if (family == MVHMR_FAMILY_SHARED) c.feature_index = reinterpret_cast<const int32_t *>(dummy);
                if (family == MVHMR_FAMILY_LENS) c.lens = dummy;
                if (family == MVHMR_FAMILY_MOMENTS) c.moments = MVHMR_MOMENTS_VAR;
                if (family == MVHMR_FAMILY_WEIGHTED) c.view_weights = dummy;
                if (family == MVHMR_FAMILY_CONFIDENCE) c.view_confidence = dummy;
                // null features: refused before any launch
                EXPECT(mvhmr_unproject_forward_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
                EXPECT(mvhmr_unproject_backward_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
                EXPECT(mvhmr_unproject_backward_geometry_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
                // features given, no workspace: the whole opening runs (refusals, plan) and stops at the workspace check
                c.features = dummy;
                EXPECT(mvhmr_unproject_forward_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_WORKSPACE);
                EXPECT(mvhmr_unproject_backward_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_WORKSPACE);
                EXPECT(mvhmr_unproject_backward_geometry_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_WORKSPACE);
                // a malformed record
                c.struct_size -= 4;
                EXPECT(mvhmr_unproject_forward_call(&d, &c, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
                EXPECT(mvhmr_unproject_call_workspace_bytes(&d, &c, MVHMR_CALL_FORWARD) == 0);
                calls += 11;
            }
    // the shims: named queries against the record's, named launches with null features
    mvhmr_unproject_call c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.family = MVHMR_FAMILY_SHARED;
    c.volumes = 3;
    EXPECT(mvhmr_unproject_backward_shared_workspace_bytes(&d, 3) == mvhmr_unproject_call_workspace_bytes(&d, &c, MVHMR_CALL_BACKWARD));
    c.family = MVHMR_FAMILY_MOMENTS;
    c.placing = MVHMR_PLACING_CUBOID;
    EXPECT(mvhmr_unproject_backward_geometry_cuboid_moments_workspace_bytes(&d) == mvhmr_unproject_call_workspace_bytes(&d, &c, MVHMR_CALL_GEOMETRY));
    EXPECT(mvhmr_unproject_forward(&d, nullptr, dummy, dummy, dummy, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
    EXPECT(mvhmr_unproject_backward_cuboid_deterministic_lens(&d, dummy, nullptr, dummy, dummy, dummy, position, sides, dummy, nullptr, nullptr, nullptr, 0,
                                                              nullptr, dummy, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
    EXPECT(mvhmr_unproject_backward_geometry_weighted(&d, dummy, nullptr, dummy, dummy, nullptr, dummy, dummy, dummy, dummy, nullptr, 0, nullptr) ==
           MVHMR_ERR_INVALID_ARGUMENT);
    EXPECT(mvhmr_unproject_forward_call(&d, nullptr, nullptr, 0, nullptr) == MVHMR_ERR_INVALID_ARGUMENT);
    printf("call record host check: %d calls, %d failures\n", calls + 6, failures);
    return failures != 0;
}
