// rl_model_rows.inc -- how the rows of a file stream through a model kernel: the one host loop of rl_model_cover, rl_model_predict_contribs,
// rl_model_predict_shap, rl_model_predict_interactions and rl_model_predict_leaf_sums.  DESIGN.md 28.
// Included at the end of rl_trainer.hip, after rl_permimp.inc and before rl_contrib.inc (it uses DevPool, StageEvents and kStageScratchDefault).
// The staged and the permuted walks (StageWalk, PermWalk) keep all rows on the device and chunk over stages and cells: they are not its business.
namespace rl {

struct RowStream {
    DevPool pool;                  // dX and whatever else the call keeps on the device for its duration
    float *dX = nullptr;           // [chunk][row_stride] the rows of the chunk under way
    int64_t chunk = 0;
    double ms = 0.0;               // device time between the upload and the copy-back, over all chunks

    // A chunk's rows and what the call keeps per row beside them (bytes_per_row in all) stay within scratch_bytes (0: kStageScratchDefault);
    // a chunk holds at least one row.
    int open(int64_t n_docs, int32_t row_stride, int64_t scratch_bytes, int64_t bytes_per_row)
    {
        const int64_t budget = scratch_bytes > 0 ? scratch_bytes : kStageScratchDefault;
        chunk = std::max<int64_t>(1, std::min<int64_t>(n_docs, budget / bytes_per_row));
        RL_HIP(pool.alloc(&dX, (size_t)chunk * row_stride));
        return RL_OK;
    }

    // Per chunk: the rows go up, launch(nr) enqueues the kernels on the null stream between two events (it returns RL_OK or the call's
    // error), and the chunk's results d_out [nr][per_row] come back to out -- a blocking copy; without d_out the device is waited for.
    // Either leaves the device idle: the next chunk overwrites dX.
    template <class T, class Launch>
    int run(const float *X, int64_t n_docs, int32_t row_stride, Launch launch, const T *d_out, T *out, int64_t per_row)
    {
        StageEvents ev;
        RL_HIP(ev.create());
        for (int64_t r0 = 0; r0 < n_docs; r0 += chunk) {
            const int64_t nr = std::min(chunk, n_docs - r0);
            RL_HIP(hipMemcpy(dX, X + (size_t)r0 * row_stride, (size_t)nr * row_stride * sizeof(float), hipMemcpyHostToDevice));
            RL_HIP(hipEventRecord(ev.e[0], 0));
            const int rc = launch(nr);
            if (rc) return rc;
            RL_HIP(hipEventRecord(ev.e[1], 0));
            if (d_out) RL_HIP(hipMemcpy(out + (size_t)r0 * per_row, d_out, (size_t)nr * per_row * sizeof(T), hipMemcpyDeviceToHost));
            else RL_HIP(hipDeviceSynchronize());
            float t = 0.f;
            RL_HIP(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
            ms += (double)t;
        }
        return RL_OK;
    }
};

}  // namespace rl
