// The `graph` block of the stand-alone harnesses' stdin (tests/test_graph_plan_host.py: describe), after the word "graph":
//   n_bufs n_ops
//   task dtype nc nk kpt_dim head_buf0 head_buf1 head_buf2 in_channels n_floats
//   level channels                                         x n_bufs
//   every field of pa_op_desc in struct order              x n_ops
#pragma once
#include <cstdio>
#include <vector>

// false: malformed.  d points into bufs / ops.
inline bool read_graph(pa_model_desc& d, std::vector<pa_buf_desc>& bufs, std::vector<pa_op_desc>& ops, long long& n_floats) {
    int nb = 0, no = 0;
    if (scanf("%d %d", &nb, &no) != 2 || nb < 0 || no < 0) return false;
    d = pa_model_desc{};
    if (scanf("%d %d %d %d %d %d %d %d %d %lld", &d.task, &d.dtype, &d.nc, &d.nk, &d.kpt_dim, &d.head_buf[0], &d.head_buf[1], &d.head_buf[2],
              &d.in_channels, &n_floats) != 10)
        return false;
    bufs.assign(nb, pa_buf_desc{});
    ops.assign(no, pa_op_desc{});
    for (auto& b : bufs) if (scanf("%d %d", &b.level, &b.channels) != 2) return false;
    for (auto& o : ops) {
        long long w_off = 0, b_off = 0;
        if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d %d", &o.kind, &o.in_buf, &o.in_choff, &o.cin, &o.out_buf, &o.out_choff,
                  &o.cout, &o.ksize, &o.stride, &o.act, &o.res_buf, &o.res_choff, &o.npad, &o.reserved, &w_off, &b_off, &o.flags, &o.pad_) != 18)
            return false;
        o.w_off = w_off; o.b_off = b_off;
    }
    d.n_bufs = nb; d.bufs = bufs.data();
    d.n_ops = no; d.ops = ops.data();
    return true;
}
