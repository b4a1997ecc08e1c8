function report = blankPulses(fileIn, fileOut, settings, threshold, pre, post, dutySamples)
% Pulse blanking of an IF record file on the GPU (DME / TACAN mitigation), to be run
% on the record BEFORE acquisition and tracking read it:
%
%   report = blankPulses(fileIn, fileOut, settings, threshold)
%   report = blankPulses(fileIn, fileOut, settings, threshold, pre, post)
%   report = blankPulses(fileIn, fileOut, settings, threshold, pre, post, dutySamples)
%
% Every sample within [m - pre, m + post] of a sample m whose amplitude exceeds
% threshold (x^2, or I^2 + Q^2 of an I/Q record, above floor(threshold^2)) is set
% to 0 in fileOut; every other byte is fileIn's, the bytes in front of
% settings.skipNumberOfBytes included, so the same settings read both files
% (settings.fileName = fileOut afterwards).  pre and post default to
% round(1e-6 * settings.samplingFreq) samples.  Five times the noise's standard
% deviation is a usual threshold; probeData's histogram shows the noise.
% settings.skipNumberOfBytes counts samples, as in tracking.  Not for fileType 3.
%
% report: n_samples, n_flagged, n_blanked, n_runs (the pulse count), threshold_sq
% and duty (blanked samples per dutySamples samples; empty without dutySamples).
if ~ischar(fileIn) || ~ischar(fileOut), error('File name must be a string'); end
if nargin < 5 || isempty(pre), pre = round(1e-6 * settings.samplingFreq); end
if nargin < 6 || isempty(post), post = round(1e-6 * settings.samplingFreq); end
if nargin < 7 || isempty(dutySamples), dutySamples = 0; end
signal = 2 - isfield(settings, 'acqCohT');   % only B1C/initSettings.m defines acqCohT: 1 = B1C, 2 = B2a
report = bds_mex('blank_pulses', fileIn, fileOut, settings, signal, threshold, pre, post, dutySamples);
fprintf('blankPulses: %d of %d samples blanked (%.1f %%) in %d runs\n', ...
        report.n_blanked, report.n_samples, 100 * report.n_blanked / max(report.n_samples, 1), report.n_runs);
end
