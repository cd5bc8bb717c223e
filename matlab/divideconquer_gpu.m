function [Sigmaout, Sigmasd, Q, logdet, Corr, Reg] = divideconquer_gpu(Y, g, k, BURNIN, MCMC, thin, rho, seed, Vprec, resp)
% DIVIDECONQUER_GPU  Sigmaout = divideconquer_gpu(Y,g,k,BURNIN,MCMC,thin,rho[,seed])
% Same arguments and output as divideconquer.m:1 (posterior-mean covariance in the
% permuted, standardised coordinates, quirk Q7), with the driver (dc:29-87) and the loop
% (dc:90-197) run by libdcfm through the dcfm_mex gateway (matlab/dcfm_mex.c):
%   dc:31-39  zero-column scan here (nnz), kept columns passed by index;
%   dc:48-59  partition + standardisation on the GPU (set_data_raw);
%   dc:68-87  initial state on the GPU from the library's Philox stream (init_state);
%   dc:90-197 the Gibbs sweep and covariance assembly (run), read back (get_sigma).
% varind = randperm(p) (dc:50) is drawn from MATLAB's stream as in the reference.
% [Sigmaout, Sigmasd] = divideconquer_gpu(...) also returns the posterior standard deviation
% of every entry of Sigma over the saved samples (same coordinates): the second moment of the
% per-sample covariance is accumulated on the GPU beside the mean (cfg.sigma_m2).
% [Sigmaout, Sigmasd, Q, logdet] = divideconquer_gpu(..., seed, Vprec) with Vprec p0 x nv (nv <= 32, one row
% per column of Y) also records Q(:,:,s) = V' * inv(Sigma_s) * V and logdet(s) = log(det(Sigma_s)) at every saved
% sample (set_precision_probes), V = Vprec(keepcols(varind), :) the block in Sigmaout's coordinates.
% [Sigmaout, Sigmasd, Q, logdet, Corr] = divideconquer_gpu(...) also returns the struct Corr with the posterior
% mean and standard deviation of the per-sample correlation matrix Sigma_s ./ sqrt(diag(Sigma_s) * diag(Sigma_s)')
% (Corr.mean, Corr.sd; Sigmaout's coordinates) and of the communalities (Corr.communality, Corr.communality_sd;
% p x 1), accumulated on the GPU beside Sigmaout (cfg.corr).
% [Sigmaout, Sigmasd, Q, logdet, Corr, Reg] = divideconquer_gpu(..., seed, Vprec, resp) with resp a list of at most
% 32 columns of Y (1-based, none of them all zero) also regresses those variables on all the others under every
% saved sample (cfg.regression, set_regression): Reg.coef and Reg.coef_sd (p x q, Sigmaout's standardised
% coordinates; y_R ~ Reg.coef' * y, the rows of the responses are 0) are the posterior mean and standard deviation
% of the coefficients Sigma_OO \ Sigma_OR, Reg.resid_cov / Reg.resid_cov_sd (q x q) those of the residual
% covariance, Reg.r2 / Reg.r2_sd (q x 1) those of R^2, Reg.count the samples behind them and Reg.responses the
% responses' rows in Sigmaout's coordinates.
if nargin < 8 || isempty(seed), seed = 0; end
if nargin < 9, Vprec = []; end
if nargin < 10, resp = []; end
[n, p0] = size(Y);
keepcols = find(arrayfun(@(j) nnz(Y(:, j)), 1:p0) > 0);   % dc:31-38
p = numel(keepcols);
P = p / g; K = k / g;
if P ~= fix(P) || K ~= fix(K)
    error('dcfm:shape', 'P = p/g = %g and K = k/g = %g must be integers (dc:41)', P, K);
end
varind = randperm(p);                                      % dc:50
cfg = struct('n', n, 'P', P, 'g', g, 'K', K, 'rho', rho, 'burnin', BURNIN, 'mcmc', MCMC, ...
             'thin', thin, 'as', 1, 'bs', 0.3, 'df', 3, 'ad1', 2, 'bd1', 1, 'ad2', 2, 'bd2', 1, ...
             'seed', seed, 'sigma_m2', double(nargout > 1), 'corr', double(nargout > 4), ...
             'regression', double(~isempty(resp)));
h = dcfm_mex('create', cfg);
cleanup = onCleanup(@() dcfm_mex('destroy', h));
dcfm_mex('set_data_raw', h, Y, int64(keepcols(varind) - 1));  % dc:48-59 on the device
dcfm_mex('init_state', h);                                     % dc:68-87 on the device
if ~isempty(Vprec), dcfm_mex('set_precision_probes', h, Vprec(keepcols(varind), :)); end
if ~isempty(resp)
    [found, rows] = ismember(resp(:)', keepcols(varind));      % the responses' rows in Sigmaout's coordinates
    if ~all(found), error('dcfm:shape', 'a response is an all-zero column of Y (dc:31-38)'); end
    dcfm_mex('set_regression', h, rows);
end
dcfm_mex('run', h, 1, BURNIN + MCMC);                          % dc:90-197
Sigmaout = dcfm_mex('get_sigma', h, p);
if nargout > 1, Sigmasd = dcfm_mex('sigma_moment', h, 'sd'); end
if nargout > 2, [Q, logdet] = dcfm_mex('precision_draws', h); end
if nargout > 4
    Corr = struct('mean', dcfm_mex('corr', h, 'mean'), 'sd', dcfm_mex('corr', h, 'sd'), ...
                  'communality', dcfm_mex('communality', h, 'mean'), ...
                  'communality_sd', dcfm_mex('communality', h, 'sd'));
end
if nargout > 5
    Reg = struct();
    if ~isempty(resp)
        [b, b2, c, c2, r, r2, cnt] = dcfm_mex('regression', h);
        Reg = struct('coef', b, 'coef_sd', sqrt(max(b2 - b.^2, 0)), 'resid_cov', c, ...
                     'resid_cov_sd', sqrt(max(c2 - c.^2, 0)), 'r2', r, 'r2_sd', sqrt(max(r2 - r.^2, 0)), ...
                     'count', cnt, 'responses', rows);
    end
end
end
