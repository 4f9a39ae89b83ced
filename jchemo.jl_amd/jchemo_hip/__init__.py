"""jchemo_hip — MI355X-native drop-in for Jchemo.jl's plskern / plsnipals hot path (host-side mirror
of the reference interface over the C ABI in include/jchemo_hip.h)."""
from ._lib import Context, JchError, LIB_PATH, SYMBOLS, default_context, load, unique_id  # noqa: F401
from .plsr import (Lwplsr, LwplsrPred, Plsr, coef, lwplsr, lwplsr_predict, query_shard, colmajor_empty, ensure_mat, plskern, plskern_, plsnipals, plsnipals_, plssimp, plssimp_, plsrosa, plsrosa_, plswold, plswold_, predict,  # noqa: F401
                   summary, transform, vip, xfit, xresid, msep, rmsep, ssr, bias, r2, cor2, segmkf, segmts, gridscorelv, gridcvlv, mpar, Plsrda, dummy, plsrda, plsrda_predict, Plslda, plslda, plsqda, plslda_predict, Mbplsr, mbplsr, mbplsr_transform, mbplsr_predict,
                   Dkplsr, dkplsr, dkplsr_, krbf, kpol, Kplsr, kplsr, kplsr_, Kpca, kpca, kpca_transform, kpca_summary)
from .krr import Krr, Krrda, gridscorelb, krr, krr_, krr_coef, krr_predict, krrda, krrda_predict  # noqa: F401
from .preproc import Savgk, detrend, detrend_, fdif, mavg, mavg_, mavg_runmean, savgk, savgol, savgol_, snv, snv_  # noqa: F401
from .covsel import Covsel, Covselr, Mlr, covsel, covsel_, covselr, covselr_coef, covselr_predict  # noqa: F401
from .pca import Pca, Pcr, pca_summary, pca_transform, pcaeigen, pcaeigen_, pcaeigenk, pcaeigenk_, pcasvd, pcasvd_, pcr, pcr_  # noqa: F401
from .robpca import colmedspa, pcasph, pcasph_, weiszfeld_step  # noqa: F401
from .occ import Occod, OccPred, Occsd, Occsdod, occ_predict, occod, occsd, occsdod, row_resid_ss  # noqa: F401
from .stah import Occstah, Stah, col_median_mad, colmad, occstah, stah  # noqa: F401
from .samp import Samp, Sampcla, Sampdp, farthest_pair, maxmin_select, sampcla, sampdp, sampks, sampsys  # noqa: F401
from .knn import (KnnPred, Knnda, Knnr, Occknndis, Occlknndis, getknn, knn_gather_median, knn_prepare, knn_release, knn_search, knn_vote, knn_wmean,  # noqa: F401
                  knnda, knnda_predict, knnr, knnr_predict, occknn_predict, occknndis, occlknndis)
from .lwmlr import (Lwmlr, LwmlrS, Lwmlrda, LwmlrdaS, knn_wls, knn_wls_lds_bytes, lwmlr, lwmlr_predict, lwmlr_s, lwmlr_s_predict, lwmlrda,  # noqa: F401
                    lwmlrda_predict, lwmlrda_s, lwmlrda_s_predict)
from .kde import Dmkern, Kernda, dmkern, dmkern_predict, kde_dens, kdeda, kdeda_predict, plskdeda, plskdeda_predict  # noqa: F401
from .gda import (Dmnorm, Lda, Qda, class_cov, dmnorm, dmnorm_predict, gauss_factor, lda, lda_predict, mahsq_chol, mahsqchol, matB, matW,  # noqa: F401
                  qda, qda_predict)
from .lwplsda import (LwplsdaPred, LwplsLda, LwplsQda, LwplsrS, Lwplsrda, LwplsrdaS, knn_gda, knn_gda_lds_bytes, locw_pspace_lds_bytes, lwplslda, lwplslda_predict,  # noqa: F401
                      lwplsqda, lwplsqda_predict, lwplsr_s, lwplsr_s_predict, lwplsrda, lwplsrda_predict, lwplsrda_s, lwplsrda_s_predict)
from .viperm import PERM_QGROUP, PERM_SLICE_ROWS, Isel, Viperm, isel, isel_intervals, perm_fill, perm_score_sums, viperm  # noqa: F401
from .plsavg import (LwplsdaAvg, LwplsrAvg, LwplsrAvgPred, lwplsravg_prepared_call, lwplsdaavg_predict, lwplsldaavg, lwplsqdaavg, lwplsravg, lwplsravg_predict, lwplsrdaavg, Plsdaavg, Plsravg, PlsravgCri, PlsravgShenk, PlsravgUnif, Plsrstack, findmax_cla, fweight, plsdaavg_predict, plsldaavg, plsqdaavg,  # noqa: F401
                     plsravg, plsravg_, plsravg_predict, plsrdaavg, row_resid_ss_lv, wshenk)
from .caltransfer import (CalDs, CalPds, calds, calds_predict, calpds, calpds_predict, difmean, eposvd, mlr, mlr_, mlr_coef, mlr_predict, mlrchol, mlrchol_,  # noqa: F401
                          mlrpinv, mlrpinv_, mlrpinvn, mlrpinvn_, mlrvec, mlrvec_, pds_table, pds_windows)
