! Batch moments of the two path tallies through the Fortran shell: computeRadiativeTransferPathMoments and reportPathMoments on the
! small cloud of levelFluxTest, six batches of 5000 photons with the seeds (/ 7, 3 ... 8 /), first with path lengths, then with the
! path histogram of pathHistogramTest (24 bins from 500 m, ratio 1.25) and three absorption coefficients.  Prints the sums and sums of
! squares over the batches -- of the domain's path figures, the column means and every column; of every bin and every coefficient --
! for tests/test_gpu_path_moments.py, which runs the same loop through the Python mirror, and what the shell answers when moments are
! asked for that were not computed, into arrays of the wrong shape, or after the kind changed.
program pathMomentsTest
  use ErrorMessages
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nPhotons = 5000, nBatches = 6, iseed = 7, firstBatch = 3, nBins = 24, nK = 3
  type(ErrorMessage)       :: status
  type(domain)             :: cloud
  type(integrator)         :: mc
  type(phaseFunction)      :: hg
  type(phaseFunctionTable) :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz), edges(nBins + 1)
  real    :: fields(nx, ny, 2, 4), wrong(nx, ny + 1, 2), means(2, 4), domainPaths(2, 4), meanFluxUp(2), meanFluxDown(2)
  real    :: bins(nBins + 1, 2, 4), spectrum(nK, 2, 4), wrongBins(nBins, 2), wrongSpectrum(nK + 1, 2)
  integer :: idx(nx, ny, nz), i, j, k, m, f, batches

  hg = new_PhaseFunction(0.85**(/ (i, i = 1, 64) /), status = status)
  table = new_PhaseFunctionTable((/ hg /), key = (/ 1. /), status = status)
  do k = 1, nz
    do j = 1, ny
      do i = 1, nx
        ext(i, j, k) = 0.0002
        if(k >= 3 .and. k <= 5) ext(i, j, k) = 0.004 * (1 + mod(i + j, 3))
      end do
    end do
  end do
  ssa = 0.95; idx = 1
  cloud = new_Domain((/ 0., 500., 1000., 1500., 2000. /), (/ 0., 500., 1000. /), (/ 0., 100., 250., 300., 500., 800., 1000. /), status)
  call addOpticalComponent(cloud, "cloud", ext, ssa, idx, table, status = status)
  mc = new_Integrator(cloud, status)
  if(stateIsFailure(status)) then
    print *, "new_Integrator failed"; stop 1
  end if
  call specifyParameters(mc, surfaceAlbedo = 0.3, minInverseTableSize = 10001, status = status)

  ! nothing computed yet; no path tally switched on
  call initializeState(status)
  call reportPathMoments(mc, domainPathUpStats = domainPaths(:, 1), status = status)
  print '(a, l2, 1x, a)', "nothingyet  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call computeRadiativeTransferPathMoments(mc, iseed, firstBatch, nBatches, 0.5, 30., nPhotons, status)
  print '(a, l2, 1x, a)', "switchedoff ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call specifyParameters(mc, status = status, absorptionCoefficients = (/ 1.e-5, -1.e-4 /))
  print '(a, l2, 1x, a)', "badspectrum ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  ! -- path lengths
  call specifyParameters(mc, status = status, computePathLengths = .true.)
  call computeRadiativeTransferPathMoments(mc, iseed, firstBatch, nBatches, 0.5, 30., nPhotons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransferPathMoments failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportPathMoments(mc, pathLengthDownStats = wrong, status = status)
  print '(a, l2, 1x, a)', "wrongshape  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportPathMoments(mc, pathHistogramUpStats = bins(:, :, 1), status = status)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportDiagnosticMoments(mc, meanLevelFluxUpStats = wrongBins(1:nz + 1, :), status = status)
  print '(a, l2, 1x, a)', "nodiagnostic", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportPathMoments(mc, pathLengthUpStats = fields(:, :, :, 1), pathLengthSquaredUpStats = fields(:, :, :, 2),           &
                         pathLengthDownStats = fields(:, :, :, 3), pathLengthSquaredDownStats = fields(:, :, :, 4),         &
                         meanPathLengthUpStats = means(:, 1), meanPathLengthSquaredUpStats = means(:, 2),                   &
                         meanPathLengthDownStats = means(:, 3), meanPathLengthSquaredDownStats = means(:, 4),               &
                         domainPathUpStats = domainPaths(:, 1), domainPathSquaredUpStats = domainPaths(:, 2),               &
                         domainPathDownStats = domainPaths(:, 3), domainPathSquaredDownStats = domainPaths(:, 4), status = status)
  if(stateIsFailure(status)) then
    print *, "reportPathMoments failed: ", trim(failureText()); stop 1
  end if
  call reportBatchMoments(mc, numBatches = batches, meanFluxUpStats = meanFluxUp, meanFluxDownStats = meanFluxDown, status = status)
  print '(a, i4)', "batches     ", batches
  print '(a, 4es16.8)', "meanflux    ", meanFluxUp, meanFluxDown
  do m = 1, 2
    print '(a, 2i3, 4es16.8)', "domainpath", m, 0, (domainPaths(m, f), f = 1, 4)
    print '(a, 2i3, 4es16.8)', "meanpath  ", m, 0, (means(m, f), f = 1, 4)
    do f = 1, 4
      print '(a, 2i3, 8es16.8)', "pathfield ", m, f, ((fields(i, j, m, f), i = 1, nx), j = 1, ny)
    end do
  end do

  ! the kind changes between the computation and the report
  call specifyParameters(mc, status = status, computePathLengths = .false.)
  call initializeState(status)
  call reportPathMoments(mc, domainPathUpStats = domainPaths(:, 1), status = status)
  print '(a, l2, 1x, a)', "switchedoff2", stateIsFailure(status), trim(failureText())
  edges(1) = 0.; edges(2) = 500.
  do i = 3, nBins + 1
    edges(i) = edges(i - 1) * 1.25
  end do
  call specifyParameters(mc, status = status, pathHistogramEdges = edges, absorptionCoefficients = (/ 1.e-5, 1.e-4, 1.e-3 /))
  call initializeState(status)
  call reportPathMoments(mc, domainPathUpStats = domainPaths(:, 1), status = status)
  print '(a, l2, 1x, a)', "otherkind   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  ! -- the path histogram and the spectrum
  call computeRadiativeTransferPathMoments(mc, iseed, firstBatch, nBatches, 0.5, 30., nPhotons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransferPathMoments failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportPathMoments(mc, domainPathDownStats = domainPaths(:, 3), status = status)
  print '(a, l2, 1x, a)', "unavailable2", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportPathMoments(mc, pathHistogramPathDownStats = wrongBins, status = status)
  print '(a, l2, 1x, a)', "wrongbins   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportPathMoments(mc, spectrumUpUpperStats = wrongSpectrum, status = status)
  print '(a, l2, 1x, a)', "wrongspectr ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportPathMoments(mc, pathHistogramUpStats = bins(:, :, 1), pathHistogramPathUpStats = bins(:, :, 2),                &
                         pathHistogramDownStats = bins(:, :, 3), pathHistogramPathDownStats = bins(:, :, 4),              &
                         spectrumUpLowerStats = spectrum(:, :, 1), spectrumUpUpperStats = spectrum(:, :, 2),              &
                         spectrumDownLowerStats = spectrum(:, :, 3), spectrumDownUpperStats = spectrum(:, :, 4), status = status)
  if(stateIsFailure(status)) then
    print *, "reportPathMoments failed: ", trim(failureText()); stop 1
  end if
  do m = 1, 2
    do f = 1, 4
      print '(a, 2i3, 25es16.8)', "bins      ", m, f, (bins(i, m, f), i = 1, nBins + 1)
      print '(a, 2i3, 3es16.8)',  "spectrum  ", m, f, (spectrum(i, m, f), i = 1, nK)
    end do
  end do
  ! other coefficients between the computation and the report; an ordinary loop afterwards forgets the path moments
  call specifyParameters(mc, status = status, absorptionCoefficients = (/ 1.e-5 /))
  call initializeState(status)
  call reportPathMoments(mc, pathHistogramUpStats = bins(:, :, 1), status = status)
  print '(a, l2, 1x, a)', "otherspectr ", stateIsFailure(status), trim(failureText())
  call specifyParameters(mc, status = status, pathHistogramEdges = edges(1:0))
  call computeRadiativeTransferBatchMoments(mc, iseed, firstBatch, 2, 0.5, 30., nPhotons, status)
  call initializeState(status)
  call reportPathMoments(mc, pathHistogramUpStats = bins(:, :, 1), status = status)
  print '(a, l2, 1x, a)', "forgotten   ", stateIsFailure(status), trim(failureText())
  call finalize_Integrator(mc)
  print '(a)', "path moments test done"
contains
  ! the newest message of the status object that says something (the probes start from a fresh one; a computation leaves the
  ! successes of its preparations in front of its failure)
  function failureText() result(text)
    character(len = 256) :: text, line
    text = ""
    call firstMessage(status)
    do while(moreMessagesExist(status))
      line = getCurrentMessage(status)
      if(len_trim(line) > 0) text = line
      call nextMessage(status)
    end do
  end function failureText
end program pathMomentsTest
