// pagk_group_sensor_kernel.h -- the stages a SENSOR sequence adds to a frame, for k cameras at once (include/pagk.h: the sensor
// form of the sequence group, pagk_sequence_group_step_sensor).  A sensor step with the FAST top-up enqueues eight or nine small
// launches per camera beside those of pagk_group_kernel.h: the rectification, the gyro integration, the hand-over's plan, the
// four of the detector, the flow velocities.  Here, as there, the camera is blockIdx.y: one launch per stage for the whole rig.
//
// A workgroup reads its camera's RigRec from a second table the lead owns (record [parity * k + camera]); everything it then
// runs is the body of its camera's own launch (the *_body functions next to the single-camera kernels) on the same arguments,
// with blockIdx.x, blockDim and threadIdx as in that launch: the same arithmetic in the same order, the same bytes.  The
// pointers of a record are rebuilt as global ones (group_global, pagk_group_kernel.h), so the bodies keep their scalar loads
// and uniform branches.
//
// Every camera reads its OWN skip word (the one its plan has written): in one step the top-up may run for one camera and not
// for another, and the skipping camera's workgroups leave whole, as in its own launch.  An exit is a whole workgroup's, the
// barriers of a body are those of one workgroup, no camera waits for another one's, and the bodies' LDS is what it is in the
// single-camera kernels.  Plain HIP C++, vector stores only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_kernels.h"
#include "pagk_detect_kernel.h"
#include "pagk_fast_kernel.h"
#include "pagk_gyro_kernel.h"
#include "pagk_group_kernel.h"

namespace pagk {

// One camera's frame of one parity, the stages pagk_group_kernel.h does not have: every pointer is fixed while the group's
// tables stand (the sequence's block, the frame slot's level 0, the context's map entries and FAST workspace).
struct RigRec {
    RectArgs rect;               // k_rectify: the camera's entries, its raw frame in its input block, its slot's level 0
    GyroArgs gyro;               // k_gyro_integrate: its window in its input block, its Rbc, Rcl and rot9
    // k_handover_plan
    int32_t cap, target_n;
    double new_point_threshold;
    const uint8_t *plan_status;
    const int32_t *plan_state;
    int32_t *plan_ctl;
    // the detector (k_fast_cells, k_fast_offsets, k_fast_gather, k_fast_tree); cells.skip and tree.skip are the camera's own word
    FastCellArgs cells;
    int32_t n_cells;
    int32_t *cell_off, *ctl;
    uint32_t *kxy;
    int32_t *kscore;
    FastTreeArgs tree;
    FlowVelocityArgs flow;       // k_flow_velocity: the key set just written, the reference set's normals, the window's times
};

#define PAGK_GROUP_GLOBAL(x) x = group_global(x)

template <int CN, bool PAIR>
__global__ void __launch_bounds__(256) k_rig_rectify(const RigRec *__restrict__ table)
{
    RectArgs a = group_global(table)[blockIdx.y].rect;
    PAGK_GROUP_GLOBAL(a.entries), PAGK_GROUP_GLOBAL(a.src), PAGK_GROUP_GLOBAL(a.dst);
    rectify_body<CN, PAIR>(a);
}

__global__ void __launch_bounds__(64) k_rig_gyro_integrate(const RigRec *__restrict__ table)
{
    GyroArgs a = group_global(table)[blockIdx.y].gyro;
    PAGK_GROUP_GLOBAL(a.win), PAGK_GROUP_GLOBAL(a.Rcl), PAGK_GROUP_GLOBAL(a.rot9);
    gyro_integrate_body(a);
}

__global__ void __launch_bounds__(1024) k_rig_handover_plan(const RigRec *__restrict__ table)
{
    const RigRec &r = group_global(table)[blockIdx.y];
    handover_plan_body(r.cap, r.target_n, r.new_point_threshold, group_global(r.plan_status), group_global(r.plan_state),
                       group_global(r.plan_ctl));
}

__global__ void __launch_bounds__(256) k_rig_fast_cells(const RigRec *__restrict__ table)
{
    FastCellArgs a = group_global(table)[blockIdx.y].cells;
    PAGK_GROUP_GLOBAL(a.img), PAGK_GROUP_GLOBAL(a.seg_xy), PAGK_GROUP_GLOBAL(a.seg_score), PAGK_GROUP_GLOBAL(a.cell_cnt);
    PAGK_GROUP_GLOBAL(a.skip);
    fast_cells_body(a);
}

__global__ void __launch_bounds__(1024) k_rig_fast_offsets(const RigRec *__restrict__ table)
{
    const RigRec &r = group_global(table)[blockIdx.y];
    fast_offsets_body(r.n_cells, group_global(r.cells.cell_cnt), group_global(r.cell_off), group_global(r.ctl),
                      group_global(r.cells.skip));
}

__global__ void __launch_bounds__(256) k_rig_fast_gather(const RigRec *__restrict__ table)
{
    const RigRec &r = group_global(table)[blockIdx.y];
    fast_gather_body(r.cells.g.seg, group_global(r.cells.cell_cnt), group_global(r.cell_off), group_global(r.cells.seg_xy),
                     group_global(r.cells.seg_score), group_global(r.kxy), group_global(r.kscore), group_global(r.cells.skip));
}

__global__ void __launch_bounds__(1024) k_rig_fast_tree(const RigRec *__restrict__ table)
{
    FastTreeArgs a = group_global(table)[blockIdx.y].tree;
    PAGK_GROUP_GLOBAL(a.ctl), PAGK_GROUP_GLOBAL(a.kxy), PAGK_GROUP_GLOBAL(a.kscore), PAGK_GROUP_GLOBAL(a.knode);
    PAGK_GROUP_GLOBAL(a.box[0]), PAGK_GROUP_GLOBAL(a.box[1]), PAGK_GROUP_GLOBAL(a.ncnt[0]), PAGK_GROUP_GLOBAL(a.ncnt[1]);
    PAGK_GROUP_GLOBAL(a.ncand[0]), PAGK_GROUP_GLOBAL(a.ncand[1]), PAGK_GROUP_GLOBAL(a.cnt4), PAGK_GROUP_GLOBAL(a.cbase);
    PAGK_GROUP_GLOBAL(a.split), PAGK_GROUP_GLOBAL(a.sortk), PAGK_GROUP_GLOBAL(a.best), PAGK_GROUP_GLOBAL(a.mask);
    PAGK_GROUP_GLOBAL(a.out_xy), PAGK_GROUP_GLOBAL(a.out_resp), PAGK_GROUP_GLOBAL(a.info), PAGK_GROUP_GLOBAL(a.skip);
    fast_tree_body(a);
}

__global__ void __launch_bounds__(256) k_rig_flow_velocity(const RigRec *__restrict__ table)
{
    FlowVelocityArgs a = group_global(table)[blockIdx.y].flow;
    PAGK_GROUP_GLOBAL(a.normal_cur), PAGK_GROUP_GLOBAL(a.normal_last), PAGK_GROUP_GLOBAL(a.index_in_last);
    PAGK_GROUP_GLOBAL(a.state), PAGK_GROUP_GLOBAL(a.win), PAGK_GROUP_GLOBAL(a.v);
    flow_velocity_body(a);
}

#undef PAGK_GROUP_GLOBAL

}  // namespace pagk
